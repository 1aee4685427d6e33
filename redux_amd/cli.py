"""Command line with the reference's interface (src/main.rs):

    python -m redux_amd.cli (-c | -d) [-i <input file>] [-o <output file>] [--block-size N] [--element-size E]
                            [--model adaptive|static|plane-static|segment-static|context-static|auto] [--segment-blocks G] [--checksum]
                            [--stored]
                            [--filter delta|zigzag|lag|stride] [--lag S|auto] [--stride S] [--order K] [--order-auto] [--record-size R|auto] [--base <base file>] [--skip-constant] [--layout auto|mixed]
                            [--range START:LENGTH] [--base-op xor|sub|auto]

Same flags, same fixed Parameters::new(8, 30, 32) (main.rs:108), same exit codes (1 usage,
2 cannot open a file, 3 coding error) and the same summary line on stderr (main.rs:112,117).
`--block-size 0` (the default) produces / expects the reference's raw single stream -- one
coder, so one GPU lane; any other value cuts the input into independent blocks coded in
parallel and wraps them in the container of redux_amd/container.py.  All coding runs on the
GPU: there is no CPU path.  `--element-size 2|4|8` (with a block size) codes typed data -- bf16 / fp16, fp32 / int32,
fp64 / int64 -- in the byte-plane layout (container version 2); decoding reads the element size from the container.
A raw reference stream has no place to record it: `--element-size` above 1 with `--block-size 0` is a usage error.
`--model static` (with a block size, element size 1) builds one static frequency table from the whole input and codes
every block under it (container version 3, which records the table); `--model adaptive`, the default, is the
reference's model.  `--model plane-static` (with a block size and `--element-size 2|4|8`) builds one static table per
byte plane of the layout and codes each plane's blocks under its own (container version 4, which records the E tables);
without a block size, with `--element-size` absent or 1, or with `--stored` it is a usage error.  Decoding reads the model
from the container.
`--model segment-static` (with a block size and any `--element-size`) builds static tables per range of G blocks of the
layout, `--segment-blocks G`, a multiple of 64 * element size (default 256 * element size), from each range as it is coded
(container version 5, which records k = G / (64 E) and the tables): the model for large inputs whose statistics drift,
such as checkpoints.  Without a block size, with `--stored`, with a G that is no such multiple, or `--segment-blocks` with
another model, it is a usage error.
`--model context-static` (with a block size, element size 1) builds a static table per preceding byte -- an order-1
model -- from the whole input and codes every byte under the table of the byte before it (container version 7, which
records the tables of the contexts that occur).  It pays on text, logs and source code from about half a megabyte upward
(bible.txt: 0.42 against 0.54) and costs up to 128 KiB of tables below that, so only `--model auto` chooses it for you.  With
`--block-size 0`, `--stored`, `--filter` or an `--element-size` other than 1 it is a usage error.
`--model auto` (with a block size and any `--element-size`) estimates the container each model would write -- adaptive and
segment-static always, static and context-static for element size 1, plane-static above -- from histograms of the input taken
on the GPU, without coding it (redux_amd/container.py: estimate_bytes), and codes with the smallest; ties go to
the earlier of adaptive, static, plane-static, segment-static, context-static.  The output is that model's container:
nothing new for -d.  The filter and stored blocks are not chosen by it (the filter and the element size are `--layout auto`'s
choice, under the adaptive model): `--model auto` with `--block-size 0`, `--stored`, `--filter` or `--segment-blocks` is a
usage error.
`--checksum` (with -c and a block size) records the CRC-32 (zlib.crc32) of every block's uncompressed bytes in the container
(version flag 0x10); -d checks every block of such a container against it, and a block that decodes to other bytes -- a
damaged, swapped or misplaced block -- is a decompression error (exit 3).  A raw reference stream has no room for the
table: `--checksum` with `--block-size 0` is a usage error.
`--stored` (with -c and a block size, adaptive model) writes a block whose stream would not be smaller than the block as
its raw bytes (container flag 0x40): incompressible data then costs no more than its own size plus the tables, and
decodes as a copy.  -d reads any stored container.  `--stored` with `--block-size 0` or a static model is a usage error.
`--filter delta` (with -c, a block size and any `--element-size`, adaptive model) codes the differences of neighbouring
little-endian unsigned elements instead of the elements, frame by frame of the byte-plane layout (container version 6):
for integer series whose values are large but close to their neighbours -- timestamps, sorted indices, offsets, counters,
sampled signals.  Floating-point data and text get larger with it, so only `--layout auto` chooses it for you.  -d reads it
from the container.  `--filter` with `--block-size 0`, `--stored` or a `--model` other than adaptive is a usage error.
`--filter zigzag` (the rules of `--filter delta`; `--checksum` is allowed) folds every difference so that small magnitudes
of either sign become small unsigned numbers (container version 11): for signed series that move both ways -- sampled
signals, random walks, offsets that go back and forth -- whose small negative differences would otherwise put 0xFF into
every upper byte plane; an int64 signal comes out at about half the size of `--filter delta`, a monotone series at the
same size.  `--layout auto` does not choose it.  -d and -d `--range` read version 11 with no flag.  With `--block-size 0`,
`--stored`, `--base`, `--skip-constant`, `--layout` or a `--model` other than adaptive it is a usage error.
`--filter lag --lag S` (the rules of `--filter zigzag`; S from 1 to 256) takes the folded difference to the element S back
instead of the one directly before (container version 13, which records S): for S interleaved channels -- stereo or
multi-channel PCM, IMU and ADC logs, (x, y, z) vertex arrays, RGB(A) pixels -- and row-major tables of records of S columns,
where the element before belongs to another series and `--filter delta` or `zigzag` makes the file larger.  On interleaved
int16 / int32 random walks it comes out at 0.54 to 0.65 of the best of plain, planes, delta and zigzag; a wrong lag costs up
to 10 % over them, so the filter stays opt-in: nothing chooses it for you, and `--layout auto` does not see it.  S can be
counted: `--filter lag --lag auto` estimates the payload behind every lag from 1 to 256 on the GPU, from the input as it
stands and without transforming or coding it (redux_amd/api.py: choose_lag), and codes with the smallest, ties
to the smaller S.  Up to 64 frames (of element size times block size bytes) that is one exact pass; above, a first pass over
about 64 evenly spaced frames, then an exact pass over every frame for the three best lags and S = 1 -- which is always among
them, so the chosen lag is never estimated above `--filter zigzag`.  The output is that lag's container, version 13, which
records it: nothing new for -d.  `--lag 1` is `--filter zigzag` under another version number.  -d
and -d `--range` read version 13 with no flag.  `--lag` without `--filter lag`, `--filter lag` without `--lag`, and an S that
is neither a decimal number from 1 to 256 nor the word `auto` are usage errors.
`--order K` (with `--filter lag --lag S`; K is 1, 2 or 3; `--checksum` is allowed) applies the lag-S difference K times
(container version 14, which records K and S): for sampled, band-limited signals -- PCM, vibration and IMU logs, ADC traces --
which are locally a low-degree polynomial, as FLAC's fixed predictors of order 2 and 3 and every "delta of delta" codec
assume.  On generated tonal signals (three sinusoids plus noise per channel) order 2 comes out at 0.72 to 0.77 and order 3 at
0.67 to 0.73 of order 1; on generated random walks, for which order 1 is already optimal, they cost 5 and 13 to 16 % more,
so the order stays opt-in and nothing chooses it for you.  No recorded signal was measured: the figures rest on generated
data.  `--order 1` is `--filter lag --lag S` itself and writes version 13, byte for byte.  -d and -d `--range` read version
14 with no flag.  `--order` without `--filter lag`, a K that is not the decimal 1, 2 or 3, and `--order 2` or `3` with
`--lag auto` (the lag estimates count order 1 only) are usage errors.
`--order-auto` (with -c and `--filter lag --lag S` or `--lag auto`; a flag without a value) counts the order too: the payload
behind orders 1, 2 and 3 is estimated on the GPU, from the input as it stands and without transforming or coding it
(redux_amd/api.py: choose_lag_order) -- at lag S, or with `--lag auto` at each of that choice's finalists, at
most 12 candidates in one exact pass -- and the smallest codes the data, ties to the smaller order, then to the smaller lag.
Order 1 is always among the candidates, so the choice is never estimated above `--filter lag --lag S|auto` alone.  The output
is that choice's ordinary container, version 13 for order 1 and version 14 above: nothing new for -d.  The figures behind it
rest on generated data as well.  `--order-auto` together with `--order`, without `--filter lag --lag ...`, with -d, or with
anything `--order 2` is refused with is a usage error.
`--base FILE` (with -c, a block size and any `--element-size`, adaptive model; `--checksum` is allowed) codes the bytewise
XOR of the input against FILE, an earlier snapshot of the same tensors -- the previous checkpoint, the base model of a
fine-tune -- in the byte-plane layout (container version 8, which records how many bytes of the base were used and their
CRC-32).  A base of another length is fine: what lies past its end is coded as it is.  With -d, `--base FILE` supplies the
base of a version 8 container: a missing, different or too short base, and a base given for any other input, is a
decompression error (exit 3).  With -c, `--base` with `--block-size 0`, `--stored`, `--filter` or any `--model` other than
adaptive (auto included: the base is never chosen for you) is a usage error; a base file that cannot be opened is exit 2.
`--base-op sub` (with -c and `--base`, so a block size, any `--element-size` and the adaptive model; `--checksum` is
allowed) codes the folded difference of the little-endian elements against the base in place of the XOR (container version
12, with version 8's base record): small where the input and the base are close as numbers, also across a carry, where XOR is
not.  On synthetic fp32 pairs it comes out 4 to 6 % below XOR, on bf16 pairs 7 to 18 %, on unrelated pairs under 1 % above
(no real checkpoint series was measured).  `--base-op auto` estimates the payload behind both operations on the
GPU, without coding, and codes with the smaller (a tie goes to XOR); the output is that operation's container, version 8 or
12.  `--base-op xor` is the default.  -d and -d `--range` read version 12 with `--base FILE` and no other flag.  `--base-op`
with -d, without `--base` or with anything `--base` refuses is a usage error, and so is `--base-op sub` or `auto` with
`--skip-constant`.
`--skip-constant` (with -c, a block size and any `--element-size`, adaptive model; `--checksum` and `--base` are allowed)
leaves every block of the coder's input whose bytes are all equal out of the coder: it travels as one byte (container
version 9) and is rebuilt by a fill.  Behind `--base` that is every unchanged region of a snapshot.  -d reads version 9
with no flag.  `--skip-constant` with `--block-size 0`, `--stored`, `--filter` or any `--model` other than adaptive is a
usage error.
`--layout auto` (with -c and a block size, adaptive model; `--checksum` is allowed) estimates the container the adaptive
coder would write behind each of the eight layouts -- element size 1, 2, 4, 8, each with and without the delta filter --
from one pass over the input as it stands on the GPU, without transforming or coding it (redux_amd/container.py:
estimate_layout_bytes), and codes with the smallest; ties go to the earlier of plain 1, 2, 4, 8, delta 1, 2, 4,
8.  With `--element-size E` the choice is between plain and delta at that E.  The output is that layout's container (version
1, 2 or 6): nothing new for -d.  `--layout auto` with `--block-size 0`, `--stored`, `--filter`, `--base`, `--skip-constant`,
-d or any `--model` other than adaptive is a usage error.
`--layout mixed` (with -c and a block size, adaptive model; `--checksum` is allowed) makes that choice for every unit of 8
blocks on its own, on the GPU, and codes each unit behind its own layout (container version 10, which records a byte per
unit): for files that hold several element types -- a checkpoint with bf16 weights next to fp32 state, int64
indices and a text header -- where one layout for the whole file can only be the least bad.  A file of one type pays one byte
per 8 blocks for it.  With `--element-size E` every unit is plain or delta at that E.  -d reads version 10 with no flag.
The usage errors are those of `--layout auto`.
`--record-size R [--filter delta]` (with -c and a block size; R from 2 to 256; `--checksum` is allowed) is the record layout
for fixed-width structs: a packed C struct dump, a numpy structured array, a row-major table.  Every block then holds one byte
column of block-size records of R bytes, and `--filter delta` with it is the byte delta against the record before, not the
integer delta filter.  On generated tables of 23- and 20-byte structs, layout and delta together come out at
about 0.74 to 0.75 of the best of plain, planes and `--filter lag`.  The output is
container version 15, which records both: -d and -d `--range` read it with no flag.  `--record-size` with -d, with
`--block-size 0`, an `--element-size` other than 1, `--stored`, a `--model` other than adaptive, `--filter zigzag` or `lag`,
`--lag`, `--order`, `--order-auto`, `--base`, `--skip-constant` or `--layout`, and an R that is neither a decimal from 2 to 256 nor
`auto`, is a usage error.
`--record-size auto` (with -c and a block size; `--checksum` is allowed) counts R and the filter for a struct dump of unknown
width (redux_amd/api.py: choose_record): all 510 candidates, R from 2 to 256 with and without the byte delta, are
costed on the GPU from the bytes as they are -- about 64 blocks of each first, then every frame for the four best and for the
plain bytes -- and the smallest estimate codes the data, unless its gain over the plain bytes is one that the smallest of 510
draws of noise explains.  The output is that choice's ordinary container, version 15, or the
plain version 1 container where the layout is estimated to cost bytes: nothing new for -d.  On the generated tables above it
finds 23 and 20 with the delta; no recorded table was measured.  `--record-size auto` with `--filter`, and with everything
`--record-size R` is a usage error with, is a usage error.
`--filter stride --stride S [--element-size E]` (with -c and a block size; S a decimal number of elements from 1 to 2^64 - 1;
`--checksum` is allowed) is for ONE file of T snapshots of the same S elements -- a trajectory [frame, atom, xyz], a field
[time, lat, lon], a stack of sensor frames, a tensor logged every step: every element is coded as its folded difference to the
same element one snapshot back, S elements earlier in the file however far that is (`--lag` ends at 256, and `--base` needs the
earlier snapshot as a second file).  On generated trajectories and sensor frames it comes out at 0.53 to 0.67 of the best of
plain, planes, zigzag and lag; on unrelated snapshots it costs about 2 %, so nothing chooses it for the caller.  The output is
container version 15, kind 2, which records S: -d reads it with no flag.  It has no range reads -- an element needs every
snapshot before it -- so -d `--range` on such a container is a usage error with a message saying so.  `--stride` without
`--filter stride`, `--filter stride` without `--stride`, an S that is no such number, and either with -d, `--block-size 0`,
`--stored`, `--lag`, `--order`, `--order-auto`, `--record-size`, `--base`, `--skip-constant`, `--layout` or a `--model` other than
adaptive are usage errors.
`--range START:LENGTH` (with -d; both decimal, START + LENGTH at most the length of the data) writes only the bytes
[START, START + LENGTH) of the original data, and decodes only the blocks that hold them (redux_amd/container.py: Reader;
DESIGN.md 6o): one tensor out of a checkpoint.  With `-i FILE` the file is not read as a whole: the header and the tables are,
then the streams of the covered blocks, so damage elsewhere in the file goes unnoticed; from stdin the input is read to its
end first.  The summary line reports the bytes written and the bytes read from the input.  `--base FILE` works as for -d.  A
raw reference stream has no random access, and a range may not leave the data: both are decompression errors (exit 3).
`--range` with -c, without a value, or with a value that is not two non-negative decimal numbers around a colon, is a usage
error.
"""
import io
import sys

USAGE = ("Usage: redux (-c | -d) [-i <input file>] [-o <output file>] [--block-size <bytes>] [--element-size <1|2|4|8>] "
         "[--model <adaptive|static|plane-static|segment-static|context-static|auto>] [--segment-blocks <G>] [--checksum] [--stored] "
         "[--filter <delta|zigzag|lag|stride>] [--lag <1..256|auto>] [--stride <S>] [--order <1|2|3>] [--order-auto] [--record-size <2..256>|auto] [--base <base file>] [--skip-constant] [--layout <auto|mixed>] [--range <start>:<length>] "
         "[--base-op <xor|sub|auto>]")


def parse(argv):
    opts = {"compress": None, "input": None, "output": None, "block_size": 0}  # (+ "element_size", "model" when given)
    it = iter(argv)
    for arg in it:
        if arg == "-c":
            opts["compress"] = True
        elif arg == "--checksum":
            opts["checksum"] = True
        elif arg == "--stored":
            opts["stored"] = True
        elif arg == "-d":
            opts["compress"] = False
        elif arg == "--skip-constant":
            opts["skip_constant"] = True
        elif arg == "--order-auto":
            if "order" in opts:
                return None  # the order is given or counted, not both
            opts["order"] = "auto"
        elif arg in ("-i", "-o", "--block-size", "--element-size", "--model", "--segment-blocks", "--filter", "--base", "--layout", "--range",
                     "--base-op", "--lag", "--order", "--record-size", "--stride"):
            val = next(it, None)
            if val is None:
                return None
            if arg == "-i":
                opts["input"] = val
            elif arg == "-o":
                opts["output"] = val
            elif arg == "--element-size":
                if val not in ("1", "2", "4", "8"):
                    return None
                opts["element_size"] = int(val)
            elif arg == "--model":
                if val not in ("adaptive", "static", "plane-static", "segment-static", "context-static", "auto"):
                    return None
                opts["model"] = val
            elif arg == "--filter":
                if val not in ("delta", "zigzag", "lag", "stride"):
                    return None
                opts["filter"] = val
            elif arg == "--lag":
                if val == "auto":
                    opts["lag"] = val
                elif not (val.isascii() and val.isdigit()) or not 1 <= int(val) <= 256:
                    return None
                else:
                    opts["lag"] = int(val)
            elif arg == "--stride":
                if not (val.isascii() and val.isdigit()) or not 1 <= int(val) < 1 << 64:
                    return None
                opts["stride"] = int(val)
            elif arg == "--order":
                if val not in ("1", "2", "3") or "order" in opts and opts["order"] == "auto":
                    return None
                opts["order"] = int(val)
            elif arg == "--record-size":
                if val == "auto":
                    opts["record_size"] = val
                elif not (val.isascii() and val.isdigit()) or not 2 <= int(val) <= 256:
                    return None
                else:
                    opts["record_size"] = int(val)
            elif arg == "--base":
                opts["base"] = val
            elif arg == "--base-op":
                if val not in ("xor", "sub", "auto"):
                    return None
                opts["base_op"] = val
            elif arg == "--range":
                start, colon, length = val.partition(":")
                if not colon or not (start.isascii() and start.isdigit() and length.isascii() and length.isdigit()):
                    return None
                opts["range"] = (int(start), int(length))
            elif arg == "--layout":
                if val not in ("auto", "mixed"):
                    return None
                opts["layout"] = val
            elif arg == "--segment-blocks":
                if not val.isdigit() or not 0 < int(val) < 1 << 32:
                    return None
                opts["segment_blocks"] = int(val)
            else:
                try:
                    opts["block_size"] = int(val)
                except ValueError:
                    return None
                if not 0 <= opts["block_size"] <= (1 << 30):  # container.MAX_BLOCK_SIZE: a usage error, not a traceback
                    return None
        else:
            return None
    if opts.get("element_size", 1) > 1 and opts["block_size"] == 0:
        return None  # a raw reference stream has no place to record the element size
    if opts.get("model") == "static" and (opts["block_size"] == 0 or opts.get("element_size", 1) != 1):
        return None  # the table lives in the container (not in a raw stream), and there is one table, not one per plane
    if opts.get("model") == "plane-static" and (opts["block_size"] == 0 or opts.get("element_size", 1) == 1):
        return None  # the tables live in the container, one per byte plane of the layout
    if opts.get("model") == "segment-static" and (opts["block_size"] == 0 or opts.get("stored")):
        return None  # the tables live in the container, and the static decoder has no table form for stored blocks
    if opts.get("model") == "context-static" and (opts["block_size"] == 0 or opts.get("stored") or opts.get("element_size", 1) != 1):
        return None  # the tables live in the container; a table per preceding byte, of the bytes as they are
    if opts.get("model") == "auto" and (opts["block_size"] == 0 or opts.get("stored") or "segment_blocks" in opts):
        return None  # the choice is recorded as the chosen model's container; stored blocks and G are not chosen (nor the filter: below)
    if "segment_blocks" in opts:
        k, r = divmod(opts["segment_blocks"], 64 * opts.get("element_size", 1))
        if opts.get("model") != "segment-static" or r or not 1 <= k < 1 << 24:
            return None  # whole wave slots of every plane: G = 64 E k, and k must fit the container's field
    if opts.get("checksum") and opts["compress"] and opts["block_size"] == 0:
        return None  # the table lives in the container (-d verifies whatever table a container has)
    if opts.get("stored") and opts["compress"] and (opts["block_size"] == 0 or opts.get("model") in ("static", "plane-static")):
        return None  # the bitmap lives in the container, and the static decoder has no table form
    if "filter" in opts and (opts["block_size"] == 0 or opts.get("stored") or opts.get("model", "adaptive") != "adaptive"):
        return None  # the filter is recorded in the container, and it sits in front of the adaptive coder only
    if ("lag" in opts) != (opts.get("filter") == "lag"):
        return None  # the lag is the lag filter's, and that filter has no default for it (`--lag auto` asks for the count)
    if opts.get("order") == "auto":
        if opts.get("filter") != "lag" or not opts["compress"]:
            return None  # the counted order is the lag filter's, and it is counted where the data is coded
    elif "order" in opts and (opts.get("filter") != "lag" or (opts["order"] > 1 and opts.get("lag") == "auto")):
        return None  # the order is the lag filter's, and the lag estimates count order 1 only
    if "base" in opts and opts["compress"] and (opts["block_size"] == 0 or opts.get("stored") or "filter" in opts
                                               or opts.get("model", "adaptive") != "adaptive"):
        return None  # the base record lives in the container, and the XOR sits in front of the adaptive coder only
    if "base_op" in opts and (not opts["compress"] or "base" not in opts or (opts["base_op"] != "xor" and opts.get("skip_constant"))):
        return None  # the operation is recorded as the container's version, and constant blocks go behind the XOR alone
    if opts.get("skip_constant") and (not opts["compress"] or opts["block_size"] == 0 or opts.get("stored") or "filter" in opts
                                      or opts.get("model", "adaptive") != "adaptive"):
        return None  # the bitmap lives in the container, and only the adaptive coder has the table form in both directions
    if "layout" in opts and (not opts["compress"] or opts["block_size"] == 0 or opts.get("stored") or "filter" in opts
                             or "base" in opts or opts.get("skip_constant") or opts.get("model", "adaptive") != "adaptive"):
        return None  # the choice is recorded as the chosen layout's container, and it is made for the adaptive coder alone
    if "record_size" in opts and (not opts["compress"] or opts["block_size"] == 0 or opts.get("element_size", 1) != 1
                                  or opts.get("stored") or opts.get("model", "adaptive") != "adaptive"
                                  or opts.get("filter", "delta") != "delta" or "order" in opts or "base" in opts
                                  or opts.get("skip_constant") or "layout" in opts):
        return None  # the record layout is recorded in the container; it stands in place of an element size, and its one filter is the byte delta
    if ("stride" in opts) != (opts.get("filter") == "stride"):
        return None  # the stride is the stride filter's, and that filter has no default for it
    if "stride" in opts and (not opts["compress"] or "order" in opts or "record_size" in opts or "base" in opts
                             or opts.get("skip_constant") or "layout" in opts):
        return None  # the stride is recorded in the container, and the filter stands alone in front of the layout
    if opts.get("record_size") == "auto" and "filter" in opts:
        return None  # the filter is counted with the record size, not given
    if "range" in opts and opts["compress"] is not False:
        return None  # a range is read, not written
    return None if opts["compress"] is None else opts


def main(argv=None):
    opts = parse(sys.argv[1:] if argv is None else argv)
    if opts is None:
        print(USAGE, file=sys.stderr)
        return 1
    ranged = "range" in opts and opts["input"] is not None  # (the input file stays open and is read piece by piece)
    try:
        data = sys.stdin.buffer.read() if opts["input"] is None else open(opts["input"], "rb") if ranged \
            else open(opts["input"], "rb").read()
    except OSError as e:
        print(f"Error while opening input file {opts['input']}: {e}", file=sys.stderr)
        return 2
    base = None
    if "base" in opts:
        try:
            base = open(opts["base"], "rb").read()
        except OSError as e:
            print(f"Error while opening base file {opts['base']}: {e}", file=sys.stderr)
            if ranged:
                data.close()
            return 2
    try:
        sink = sys.stdout.buffer if opts["output"] is None else open(opts["output"], "wb")
    except OSError as e:
        print(f"Error while opening output file {opts['output']}: {e}", file=sys.stderr)
        if ranged:
            data.close()
        return 2

    from . import api, container
    params = api.Parameters.new(8, 30, 32)  # main.rs:108
    try:
        if opts["compress"]:
            if opts["block_size"] == 0:
                o = io.BytesIO()
                i_n, o_n = api.compress(io.BytesIO(data), o, api.AdaptiveTreeModel.new(params))
                sink.write(o.getvalue())
            else:
                # (--layout auto / mixed without --element-size: element size None, the choice among all eight layouts)
                blob = container.compress_bytes(data, opts["block_size"], params,
                                                opts.get("element_size", None if "layout" in opts else 1),
                                                opts.get("model", "adaptive"), opts.get("checksum", False),
                                                opts.get("stored", False), opts.get("segment_blocks"), opts.get("filter"), base,
                                                opts.get("skip_constant", False), opts.get("layout"), opts.get("stride"),
                                                opts.get("record_size"),
                                                opts.get("lag"), opts.get("order"), opts.get("base_op", "xor"))
                sink.write(blob)
                i_n, o_n = len(data), len(blob)
            print("Compressed %d bytes into %d bytes, ratio: %.3f" % (i_n, o_n, i_n / o_n), file=sys.stderr)
        elif "range" in opts:
            # (a raw reference stream has no random access: what is no container fails the header's checks here)
            reader = container.Reader(data, base)
            if reader.stride is not None:  # (known only once the header is read: a usage error all the same)
                print("--range: a container of --filter stride has no range reads (an element needs every snapshot before "
                      "it); decode it whole with -d", file=sys.stderr)
                print(USAGE, file=sys.stderr)
                return 1
            out = reader.read(*opts["range"])
            sink.write(out)
            i_n, o_n = reader.bytes_read, len(out)
            ratio = (o_n / i_n) if i_n else float("nan")
            print("Decompressed %d bytes from %d bytes read, ratio: %.3f" % (o_n, i_n, ratio), file=sys.stderr)
        else:
            # A container is recognised by a well-formed HEADER, not by its magic alone: a raw reference
            # stream may begin with the same four bytes.  Once the header is consistent the input IS a
            # container: a truncated or damaged body is reported as such (exit 3), not decoded as garbage.
            is_container = container.header_is_wellformed(data)
            if is_container:
                out = container.decompress_bytes(data, base)
                sink.write(out)
                i_n, o_n = len(data), len(out)
            else:
                if base is not None:  # (a raw reference stream was not written against a base)
                    raise api.InvalidInput()
                o = io.BytesIO()
                i_n, o_n = api.decompress(io.BytesIO(data), o, api.AdaptiveTreeModel.new(params))
                sink.write(o.getvalue())
            ratio = (o_n / i_n) if i_n else float("nan")
            print("Decompressed %d bytes from %d bytes, ratio: %.3f" % (o_n, i_n, ratio), file=sys.stderr)
    except api.Error as e:
        print(("Compression" if opts["compress"] else "Decompression") + f" error: {e}", file=sys.stderr)
        return 3
    finally:
        if opts["output"] is not None:
            sink.close()
        if ranged:
            data.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
