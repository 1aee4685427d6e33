/*
 * redux_hip.h -- C ABI of the MI355X-native block coder that sits behind peterbudai/redux's
 * compress / decompress surface.  Plain pointers and sizes only; no HIP or torch types.
 *
 * Every entry point names the reference interface it replaces (file:line under the
 * reference checkout).  The reference-side binding a maintainer would add (Rust
 * `extern "C"` block + safe wrappers) is shown in INTEGRATION.md.
 *
 * Semantics shared by all calls
 *   - A "block" is block_size consecutive input bytes (the last one may be shorter; an
 *     empty input is ONE empty block).  Each block is coded by a fresh Codec + fresh
 *     AdaptiveTreeModel, so block b's stream is byte-identical to
 *     redux::compress(&mut &in[b*block_size..], .., AdaptiveTreeModel::new(params))
 *     (src/lib.rs:102, src/codec.rs:104, src/model/adaptive_tree.rs:36).
 *   - Status codes mirror src/lib.rs:57-64: 0 Ok, 1 Eof, 2 InvalidInput, 3 IoError (here: a
 *     HIP runtime failure), plus 4 OutputTooSmall and 5 Unsupported (parameters the device
 *     path does not implement: symbol_bits > 16; symbol_bits == 8 with code_bits <= 32 runs on
 *     the fast kernels, 4- and 12-bit symbols with code_bits <= 32 on lock-step kernels of the
 *     same form, every other valid triple on a one-lane-per-block kernel).  There is NO
 *     CPU fallback: Unsupported is returned, never silently served by other code.
 *   - The caller owns every buffer.  Host-pointer calls are synchronous.  `_dev` calls take
 *     device pointers, enqueue on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream), never allocate, never synchronise and keep no pointer after they return.
 *   - Thread-safe.  The `_dev` calls and the geometry helpers keep no state at all.  The
 *     host-pointer calls share ONE lazily created, mutex-guarded context per device (chunk slots
 *     in HBM, pinned staging, streams; grown on demand, buffers above 1 GiB given back when their call ends, freed by
 *     redux_host_release()): calls from several host threads are safe; two that use the same
 *     context run one after the other, two on different devices run concurrently.
 *   - The `_dev` calls launch on HIP's CURRENT device; every pointer must belong to it.
 */
#ifndef REDUX_HIP_H
#define REDUX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/lib.rs:57-64 enum Error (+ two codes the block API needs) */
enum {
    REDUX_OK               = 0,
    REDUX_EOF              = 1, /* Error::Eof: compressed input ended early (bitio/mod.rs:107) */
    REDUX_INVALID_INPUT    = 2, /* Error::InvalidInput (model/mod.rs:65, adaptive_tree.rs:131) */
    REDUX_IO_ERROR         = 3, /* Error::IoError: here a HIP runtime error */
    REDUX_OUTPUT_TOO_SMALL = 4, /* the caller's output buffer / slot cannot hold the result */
    REDUX_UNSUPPORTED      = 5  /* valid Parameters the device path does not implement */
};

/* The three integers of model::Parameters::new (src/model/mod.rs:63); the library derives
 * the other eight fields (mod.rs:67-79) itself. */
typedef struct redux_params {
    uint32_t symbol_bits; /* 1..16 on the device (8: fast kernels) */
    uint32_t freq_bits;
    uint32_t code_bits;   /* <= 32 with symbol_bits 8: fast kernels; else general path */
} redux_params;

/* One entry of a block table (the `_v` calls below): which bytes a block is, and which entry of the
 * per-block result tables is its.  16 bytes, host or device memory. */
typedef struct redux_block {
    uint64_t offset; /* encode: the block's first byte in the input buffer; decode: where its output starts */
    uint32_t length; /* encode: bytes in the block (<= block_size); decode: output capacity (<= block_size) */
    uint32_t index;  /* the block's number: its entry in out_offsets / in_offsets / out_sizes / block_status;
                        REDUX_BLOCK_IDLE: no block, the lane idles (padding, see redux_block_table_v) */
} redux_block;
#define REDUX_BLOCK_IDLE 0xFFFFFFFFu

/* model::Parameters::new validation, src/model/mod.rs:64: OK or INVALID_INPUT. */
int redux_params_check(uint32_t symbol_bits, uint32_t freq_bits, uint32_t code_bits);
/* OK, INVALID_INPUT, or UNSUPPORTED for valid triples outside the device path. */
int redux_device_supports(const redux_params *p);

/* Geometry of the block API. */
uint64_t redux_block_count(uint64_t in_len, uint32_t block_size); /* max(1, ceil(in_len / block_size)) */
/* Worst-case bytes of one block's stream for these parameters (9 bits/symbol while the model
 * cannot freeze inside a block, freq_bits+2 bits/symbol once it can, + 1 KiB). */
uint64_t redux_encode_slot_bytes(const redux_params *p, uint32_t block_size);
/* Dense-output capacity that always suffices: block_count * slot_bytes. */
uint64_t redux_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size);
/* Workspace of an encode call on the device: the blocks' slots, the reciprocal table and -- for launches the small-grid
 * kernels take -- the (low, high) pairs: 8 bytes per input byte for at most 2048 blocks of up to 64 KiB; for at most 24,576
 * blocks above 64 KiB (one block of any length included: redux_compress) TWO windows of at most 65,504 symbols per block
 * (1 MiB), at most 2816 MiB in all, because such blocks are coded window by window, the model of one window next to the
 * coder of the one before: the workspace of a long stream is its slot (9/8 of its length) + 2 MiB, whatever its length. */
uint64_t redux_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_decode_workspace_bytes(const redux_params *p, uint64_t nblocks, uint32_t block_size);

/* ---- host-pointer, synchronous ------------------------------------------------------
 * Inside, a call is a pipeline over chunks of whole blocks (~64 MiB): CPU threads stage the
 * caller's bytes into pinned memory, H2D, the chunk's kernels on its own stream, D2H -- so the
 * transfers of later chunks hide under the kernels of earlier ones (redux_amd/csrc/redux_host.hpp).
 * No hipMalloc / hipHostMalloc happens in the steady state (same or smaller shapes than before).
 *
 * redux_encode_blocks: replaces one redux::compress call per block (src/lib.rs:102-109).
 *   out          dense concatenation of the per-block streams
 *   out_offsets  nblocks+1 entries; block b's stream is out[out_offsets[b] .. out_offsets[b+1])
 *                (so (bytes_in, bytes_out) of lib.rs:108 = (block length, offsets[b+1]-offsets[b]))
 *   block_status nblocks entries, per-block status (may be NULL)
 * Returns the first non-OK per-block status, or a call-level error. */
int redux_encode_blocks(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status);

/* redux_decode_blocks: replaces one redux::decompress call per block (src/lib.rs:113-120).
 *   in / in_offsets  dense streams as produced by redux_encode_blocks
 *   out              block b is written at out + b*block_size (at most block_size bytes)
 *   out_sizes        nblocks entries: decoded length of each block
 * Per-block status: EOF for a truncated stream, INVALID_INPUT for a code value outside the
 * model's total, OUTPUT_TOO_SMALL if a (corrupt) stream decodes past block_size.
 * Block b's range [in_offsets[b], in_offsets[b+1]) may hold any number of bytes after its stream: they are
 * ignored, as redux::decompress ignores what follows its stream.  This holds for every decode call here (the
 * `_dev`, `_v`, `_crc`, planes, stored and static ones, and redux_decompress's in_len). */
int redux_decode_blocks(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks,
                        uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                        int32_t *block_status);

/* ---- many independent inputs in one call ("_v": a vector of inputs) ----------------------
 * The reference's harness codes every file by itself, one redux::compress / decompress per file
 * (tests/corpora.rs:32-85).  These calls do that for `ninputs` inputs at once: input i is the
 * bytes in[in_off[i] .. in_off[i] + in_len[i]) and is cut into blocks of block_size ON ITS OWN
 * (its last block may be shorter; an empty input is one empty block), so every block's stream
 * equals the one redux_encode_blocks produces when it is called for that input alone.  Blocks
 * are numbered input by input: input i owns blocks first(i) .. first(i) + redux_block_count(
 * in_len[i], block_size) - 1, first(0) = 0.  One launch codes all of them.
 *
 * redux_block_count_v   total number of blocks.
 * redux_block_table_v   the block table of these inputs in LAUNCH order.  A wave (64 consecutive
 *                       entries) runs its fast path for as long as its SHORTEST block lasts, so
 *                       the table puts whole blocks first, 64 to a wave, then the shorter ones by
 *                       decreasing length, and starts a new wave wherever the length has dropped
 *                       by an eighth: the rest of the old wave is filled with IDLE entries
 *                       (index = REDUX_BLOCK_IDLE; on a chip with 1024 wave slots a batch of a
 *                       few hundred blocks has lanes to spare).  entry.index = the block's number
 *                       otherwise.  Returns the number of ENTRIES (>= blocks); `table` may be
 *                       NULL (count only).
 * redux_encode_blocks_v out / out_offsets (total blocks + 1) / block_status (may be NULL) as in
 *                       redux_encode_blocks, in block-number order.
 * redux_decode_blocks_v the inverse: in / in_offsets as produced above; input i's blocks are
 *                       written to out[out_off[i] ..) back to back, at most out_len[i] bytes
 *                       (a block of input i may hold min(block_size, what is left of out_len[i]));
 *                       out_sizes / block_status per block.
 * Device path: symbol_bits == 8 and code_bits <= 32 (other valid triples: REDUX_UNSUPPORTED from
 * these calls only -- call redux_encode_blocks per input instead). */
uint64_t redux_block_count_v(const uint64_t *in_len, uint64_t ninputs, uint32_t block_size);
uint64_t redux_block_table_v(const uint64_t *in_off, const uint64_t *in_len, uint64_t ninputs, uint32_t block_size,
                             redux_block *table);
int redux_encode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                          uint64_t ninputs, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                          int32_t *block_status);
int redux_decode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint8_t *out,
                          const uint64_t *out_off, const uint64_t *out_len, uint64_t ninputs, uint32_t block_size,
                          uint32_t *out_sizes, int32_t *block_status);

/* Whole-stream drop-ins for redux::compress / redux::decompress (src/lib.rs:102,113): the
 * input is ONE block of any length, so the stream equals the reference's for the same bytes.
 * One coder = one chain of dependent symbols: correct but serial (the model is computed by a wave, the
 * interval chain by one lane; the decoder is one wave per stream); the block API is the accelerated path.
 * bytes_in / bytes_out are the (u64,u64) the reference returns.
 * LIMIT: one block is at most 0xFFFFFF00 bytes (symbol index, byte offsets and the consumed-bit count of a lane
 * are 32-bit in the kernels): redux_compress returns REDUX_UNSUPPORTED for a longer input, redux_decompress
 * clamps out_cap to it (a stream that decodes to more comes back REDUX_OUTPUT_TOO_SMALL).  The reference takes
 * any io::Read (src/lib.rs:102); a caller with more than 4 GiB in ONE stream has no parallelism to gain here
 * (~10 MB/s against ~14 MB/s for one CPU thread) and should use the block API or the CPU. */
int redux_compress(const redux_params *p, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                   uint64_t *bytes_in, uint64_t *bytes_out);
int redux_decompress(const redux_params *p, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *bytes_in, uint64_t *bytes_out);

/* Several GPUs behind the host-pointer calls.  By default a call runs on HIP's current device.
 * redux_host_set_devices(ids, n) (n <= 16; n = 0: back to the default) makes every later
 * redux_encode_blocks / redux_decode_blocks deal its chunks round-robin over n contexts, context i on
 * device ids[i] -- chunk k goes to context k mod n -- each with its own streams, HBM slots and
 * pinned staging, each fed over its own PCIe link by its own host threads; the data starts and ends
 * in host memory, so the devices exchange nothing (no collective).  An id may appear more than once
 * (two contexts on one device: what the one-GPU test box exercises).  The `_v` calls deal their GROUPS of inputs
 * (512 MiB of payload each) the same way, group k on context k mod n.
 * Existing contexts are released by the call.  Returns INVALID_INPUT for an id that is not a device.
 * redux_host_chunk_plan: the chunking such a call uses for nblocks blocks on ncontexts contexts
 * (whole waves of 64 blocks per chunk); host arithmetic only.
 * redux_host_set_chunk_bytes: overrides the chunk size limits (bytes of payload per chunk; 0, 0 = the
 * defaults, 16 MiB .. 128 / 256 MiB): a harness uses it to drive many chunks through a small input. */
int  redux_host_set_devices(const int32_t *device_ids, uint32_t n);
int  redux_host_chunk_plan(uint64_t nblocks, uint32_t block_size, uint32_t ncontexts, int decode, uint64_t *chunk_blocks,
                           uint64_t *nchunks);
int  redux_host_set_chunk_bytes(uint64_t min_bytes, uint64_t max_bytes);

/* Frees every per-device context of the host-pointer calls (they are rebuilt on the next call).
 * redux_host_allocations: hipMalloc + hipHostMalloc calls the contexts have made so far -- a
 * harness checks that it does not move in the steady state. */
int      redux_host_release(void);
uint64_t redux_host_allocations(void);
/* Device memory the contexts hold right now, in bytes.  A context keeps what the chunk pipeline can ask for and gives
 * back slot buffers above 1 GiB when the call that needed them ends (one block of hundreds of MiB, a generous decode
 * capacity); the decoders' workspace does not grow with the capacity at all (a bounded reciprocal table). */
uint64_t redux_host_resident_bytes(void);
/* Diagnostic: the timeline of the last host-pointer call on the current device, four doubles per
 * chunk (seconds since the call began): staging begins, device work enqueued, kernels done, results
 * in caller memory.  Copies up to cap doubles, returns how many there are. */
uint64_t redux_host_trace(double *out, uint64_t cap);

/* ---- device-pointer, stream-ordered --------------------------------------------------
 * Same contracts with every pointer in device memory.  d_workspace must hold
 * redux_encode_workspace_bytes() / redux_decode_workspace_bytes() bytes and be 256-B aligned.
 * d_summary (int32[2], may be NULL): [0] = first non-OK status over all blocks (0 if none),
 * [1] = number of non-OK blocks.  Errors found on the device are reported there and in
 * d_block_status; the return value covers argument and launch errors only. */
int redux_encode_blocks_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                            void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_blocks_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                            uint64_t nblocks, uint32_t block_size, void *d_out, uint64_t out_cap,
                            void *d_out_sizes /* u32[nblocks] */, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);

/* The `_v` calls with everything in device memory.  d_table: redux_block[nentries] in launch order
 * (redux_block_table_v builds one; any order is valid, a wave's 64 consecutive entries run in
 * lock-step for as long as its shortest block lasts).  The table is CHECKED on the device before any
 * coder kernel reads it (one thread per entry, tens of microseconds; the kernels then read a copy in the
 * workspace, the caller's table is never written): an entry must be idle (index REDUX_BLOCK_IDLE) or have
 * index < nblocks, an index no other entry has, length <= block_size, offset + length <= in_bytes /
 * out_bytes and, under REDUX_V_ALIGNED16, offset a multiple of 16.  An entry that fails is treated as
 * idle -- nothing is read or written through it --, a block that no valid entry codes comes back with
 * size 0 and status REDUX_INVALID_INPUT, and d_summary[0] is REDUX_INVALID_INPUT (the return value covers
 * argument and launch errors only, as everywhere: the call is stream-ordered).  As the reference's
 * surface never writes out of bounds (bitio/mod.rs:148-198 returns Err), neither does a bad table.  Encode: entry.offset is the block's first
 * byte in d_in (in_bytes = size of that buffer, below 4 GiB), entry.length its size.  Decode:
 * entry.offset is where the block's output starts in d_out (out_bytes = size of that buffer),
 * entry.length the room it has there.  flags: REDUX_V_ALIGNED16 promises that d_in / d_out and
 * every entry.offset are multiples of 16 (the fast kernels need it; without it the call is
 * correct and slow).  nentries = entries of the table (idle ones included), nblocks = blocks.
 * Workspace: redux_encode_workspace_bytes(p, nentries * block_size, block_size) /
 * redux_decode_workspace_bytes(p, nentries, block_size). */
enum { REDUX_V_ALIGNED16 = 1 };
int redux_encode_blocks_v_dev(const redux_params *p, const void *d_in, uint64_t in_bytes, const void *d_table,
                              uint64_t nentries, uint64_t nblocks, uint32_t block_size, uint32_t flags, void *d_out,
                              uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */, void *d_block_status /* i32[nblocks] */,
                              void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_blocks_v_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                              const void *d_table, uint64_t nentries, uint64_t nblocks, uint32_t block_size, uint32_t flags,
                              void *d_out, uint64_t out_bytes, void *d_out_sizes /* u32[nblocks] */, void *d_block_status,
                              void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* The two phases of redux_encode_blocks_dev, exposed so a harness can time the coder kernel
 * by itself: (1) code every block into its padded slot inside the workspace and record the
 * sizes; (2) scan the sizes and gather the slots into the dense output.  Both take the same
 * (in_len, block_size, d_workspace, workspace_bytes): the layout inside the workspace is a function of
 * the shape AND of workspace_bytes (a workspace without room for the small-launch kernels' pairs area
 * makes a small launch run the full-grid kernels on their layout), so the phases must be told the same. */
int redux_encode_slots_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                           void *d_block_status, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_compact_slots_dev(const redux_params *p, uint64_t in_len, uint32_t block_size, void *d_out, uint64_t out_cap,
                            void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);

/* ---- synthetic workloads of BASELINE.json, generated in HBM ----------
 * iid : byte j = byte (j mod 8), little-endian, of splitmix64(seed + j/8).
 * zipf: byte j = rank-1 where rank is drawn by inverse CDF of P(r) ~ r^-1.2, r = 1..256,
 *       from the high 32 bits of splitmix64(seed + j) against the 256-entry u32 table
 *       returned by redux_zipf_thresholds() (thresholds[r-1] = floor(2^32 * CDF(r)) , last = 2^32-1).
 * first_byte lets a rank generate its own shard: byte j of the call is stream byte first_byte + j. */
int redux_gen_iid_dev(void *d_out, uint64_t len, uint64_t first_byte, uint64_t seed, void *stream);
int redux_gen_zipf_dev(void *d_out, uint64_t len, uint64_t first_byte, uint64_t seed, void *stream);
const uint32_t *redux_zipf_thresholds(void);

/* ---- static-table model ------------------------------------------
 * The reference's Codec is generic over its Model trait (src/model/mod.rs; lib.rs:14-15 invites
 * custom models).  The cheapest second model is a fixed table: cum[0..=257] (host memory, 258
 * entries) with cum[0] = 0, cum strictly increasing and cum[257] = total_frequency() <= freq_max.
 * get_frequency(s) = [cum[s], cum[s+1]) for the data symbols 0..255 and for EOF = 256; nothing is
 * updated.  Block b's stream is Codec::compress_stream (codec.rs:104-120) of that block under
 * such a model.  Device path: symbol_bits == 8, code_bits <= 32 (else REDUX_UNSUPPORTED); a table
 * that is not strictly increasing or exceeds freq_max is REDUX_INVALID_INPUT.
 * Same buffers and error reporting as redux_encode_blocks_dev / redux_decode_blocks_dev. */
int      redux_static_table_check(const redux_params *p, const uint32_t *cum);
uint64_t redux_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size);
int redux_static_encode_blocks_dev(const redux_params *p, const uint32_t *cum, const void *d_in, uint64_t in_len,
                                   uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                                   void *d_block_status, void *d_summary, void *d_workspace,
                                   uint64_t workspace_bytes, void *stream);
int redux_static_decode_blocks_dev(const redux_params *p, const uint32_t *cum, const void *d_in,
                                   const void *d_in_offsets, uint64_t nblocks, uint32_t block_size, void *d_out,
                                   uint64_t out_cap, void *d_out_sizes, void *d_block_status, void *d_summary,
                                   void *stream);

/* ---- semi-static coding: the static table built from the data ---------------------------------
 * The rule that turns byte counts c[0..255] into cum[0..=257] for a target total T.  The host function, the device kernel
 * and every binding agree on it bit for bit:
 *   - 257 <= T <= freq_max (else INVALID_INPUT); N = sum c; R = T - 257.  N R >= 2^64, or N >= 2^64, is
 *     UNSUPPORTED (at T = 2^16: inputs of 256 TiB or more).  Parameters the static coder does not take
 *     (symbol_bits != 8, code_bits > 32) return what redux_static_table_check returns for them.
 *   - EOF (symbol 256) always has frequency 1.  N = 0: every frequency is 1 and the total is 257.
 *   - Otherwise f[s] = 1 + floor(c[s] R / N) with remainder r[s] = c[s] R mod N; D = T - sum f (EOF included) lies in
 *     [0, 255], and the D bytes with the largest r[s] get one more (equal remainders: the lower symbol first).  Then
 *     sum f = T exactly.  cum[0] = 0, cum[i+1] = cum[i] + f[i].
 * Callers above the C ABI default to T = min(2^16, freq_max): such a table decodes on the lookup decoder.
 *
 * redux_static_table_from_counts  the rule on the host; needs no GPU.
 * redux_histogram_workspace_bytes workspace redux_histogram_dev needs for in_len bytes: 0 = none (pass NULL, 0).
 * redux_histogram_dev             ADDS the byte counts of d_in[0 .. in_len) (any length, any alignment) to d_counts, u64[256]
 *                                 on the device, stream-ordered: a buffer can be counted in pieces.  Zero the counts first.
 * redux_static_table_dev          the rule on the device: one workgroup reads d_counts (u64[256]) and writes d_cum
 *                                 (u32[258]), stream-ordered.  The parameter and total checks are made before the launch;
 *                                 N R >= 2^64 cannot be seen then, and the kernel writes a table of zeros instead, which
 *                                 redux_static_table_check rejects.
 * redux_static_table              host pointers: counts `in` on the CURRENT device (chunks staged through the host
 *                                 pipeline's pinned ring; redux_host_set_devices is ignored by this call), applies the rule
 *                                 and returns cum in host memory.
 * redux_static_encode_blocks      redux_encode_blocks / redux_decode_blocks under the table cum, through the same chunk
 * redux_static_decode_blocks      pipeline (fleet included).  Block b's stream is that of redux_static_encode_blocks_dev; the
 *                                 streams depend on neither the chunk size nor the devices.  The byte-plane form, a table
 *                                 per plane, is "plane-static coding" below. */
int      redux_static_table_from_counts(const redux_params *p, const uint64_t *counts, uint32_t total, uint32_t *cum);
uint64_t redux_histogram_workspace_bytes(uint64_t in_len);
int      redux_histogram_dev(const void *d_in, uint64_t in_len, void *d_counts /* u64[256], ADDED to */, void *d_workspace,
                             uint64_t workspace_bytes, void *stream);
int      redux_static_table_dev(const redux_params *p, const void *d_counts, uint32_t total, void *d_cum /* u32[258] */,
                                void *stream);
int      redux_static_table(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t total, uint32_t *cum);
int      redux_static_encode_blocks(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                    uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                    int32_t *block_status);
int      redux_static_decode_blocks(const redux_params *p, const uint32_t *cum, const uint8_t *in,
                                    const uint64_t *in_offsets, uint64_t nblocks, uint32_t block_size, uint8_t *out,
                                    uint64_t out_cap, uint32_t *out_sizes, int32_t *block_status);

/* ---- byte-plane layout of typed data ("shuffle" filter) ----------------------------------------
 * An order-0 byte model sees the bytes of bf16 / fp32 / int64 data interleaved: the skewed exponent byte is mixed with
 * mantissa bytes that are close to uniform.  These calls put a byte transform in front of the coder that makes each BLOCK
 * hold one byte plane.  E = element_size, one of 1, 2, 4, 8 (1 = no layout: results identical to the plain calls);
 * B = block_size.
 *   - The input is cut into frames of E*B bytes; only the last may be shorter.  A frame of L bytes holds N = L / E
 *     elements; byte p of element i moves to frame offset p*N + i; the L - N*E trailing bytes stay at the end unchanged.
 *   - So a full frame is exactly E blocks, block j of the frame being plane j of B elements.  The block cut, the streams
 *     and the container are then exactly those of the plain calls applied to the transformed bytes:
 *     stream_E(x)[b] == redux_encode_blocks(planes_E(x))[b].
 * (The adaptive model's cost of a block is the same for any order of its bytes: shuffling INSIDE a block gains nothing.)
 * Not available for the `_v` calls and redux_compress / redux_decompress; with the static-table model it is "plane-static
 * coding" below.
 *
 * redux_planes_check          OK for 1, 2, 4, 8, else INVALID_INPUT.
 * redux_planes_dev            the transform (inverse = 0) or its inverse (inverse != 0) of len bytes, d_src -> d_dst (device
 *                             buffers that must not overlap), stream-ordered.
 * redux_encode_planes_dev     redux_encode_blocks_dev of the transformed input.  The transformed copy is carved from the
 *                             FRONT of the workspace (redux_encode_planes_workspace_bytes; E = 1: the plain call's workspace).
 * redux_decode_planes_dev     the inverse: nblocks = redux_block_count(out_len, block_size) streams, block b must decode to
 *                             min(block_size, out_len - b*block_size) bytes -- one that comes back OK with another size is
 *                             reported INVALID_INPUT (and counted in d_summary) --, the blocks decode into a plane buffer in
 *                             the workspace and the inverse transform writes d_out[0 .. out_len); no byte outside that
 *                             range is written, for damaged streams too.  Every frame whose blocks are all OK holds the
 *                             original bytes.  d_out_sizes / d_block_status: nblocks entries.
 * redux_encode_blocks_planes  host-pointer forms through the same chunk pipeline as redux_encode_blocks /
 * redux_decode_blocks_planes  redux_decode_blocks (chunks are whole 64-block waves, so whole frames: the output depends on
 *                             neither the chunk size nor the devices of redux_host_set_devices); decode writes out[0 .. out_len).
 */
int      redux_planes_check(uint32_t element_size);
int      redux_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                          void *stream);
uint64_t redux_encode_planes_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_planes_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_planes_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_planes_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                            void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_planes(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                               uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status);
int redux_decode_blocks_planes(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status);

/* ---- delta filter for integer series -----------------------------------------------------------
 * Typed data whose values are large but whose neighbours are close -- timestamps, sorted indices, offsets, counters, sampled
 * signals -- has uniform low byte planes; the differences of neighbouring elements do not.  These calls put the delta
 * filter in front of the byte-plane layout (Blosc, HDF5 and Zarr ship one next to their shuffle filter).  Strictly opt-in:
 * floating-point data and plain bytes get LARGER with it.  E = element_size, one of 1, 2, 4, 8; B = block_size.
 *   - The input is cut into the frames of the byte-plane layout: E*B bytes, only the last may be shorter (E = 1: a frame
 *     is one block).  A frame of L bytes holds N = L / E little-endian unsigned elements x[0 .. N).
 *   - The filter writes d[0] = x[0] and d[i] = x[i] - x[i-1] mod 2^(8E); the L - N*E trailing bytes are unchanged.
 *   - The byte-plane layout above is then applied to the d's (E = 1: no layout).
 *   - The inverse undoes the layout and takes the running sum mod 2^(8E) inside each frame.
 * Every frame starts afresh: blocks of different frames stay independent, and a chunk boundary of the host calls changes
 * nothing (chunks are whole 64-block waves, so whole frames).  Behind the transform is the plain adaptive coder:
 *     stream_delta_E(x)[b] == redux_encode_blocks(planes_E(delta_E(x)))[b].
 * Not available with the static-table models, stored blocks, the `_v` calls and redux_compress / redux_decompress.
 *
 * redux_delta_check          OK for 1, 2, 4, 8, else INVALID_INPUT.
 * redux_delta_planes_dev     filter + layout (inverse = 0) or their inverse (inverse != 0) of len bytes, d_src -> d_dst
 *                            (device buffers that must not overlap: INVALID_INPUT), stream-ordered, one read and one write.
 * redux_encode_delta_dev     redux_encode_blocks_dev of the transformed input, the transformed copy carved from the FRONT of
 *                            the workspace (redux_encode_delta_workspace_bytes: for E = 1 too, the filter changes the bytes).
 * redux_decode_delta_dev     redux_decode_planes_dev's procedure: the blocks decode into a plane buffer in the workspace, a
 *                            block that comes back OK with another size than its place gives it is reported INVALID_INPUT,
 *                            the inverse writes d_out[0 .. out_len) and no byte outside it, for damaged streams too.  Every
 *                            frame whose blocks are all OK holds the original bytes.
 * redux_encode_blocks_delta  host-pointer forms on the chunk pipeline of redux_encode_blocks / redux_decode_blocks; the
 * redux_decode_blocks_delta  output depends on neither the chunk size nor the devices of redux_host_set_devices.  block_crc
 *                            may be null; else u32[nblocks], the CRC-32 of every block's ORIGINAL bytes ("per-block CRC-32
 *                            checksums" below: decode fills it with the CRC of what the block's range of out holds).
 */
int      redux_delta_check(uint32_t element_size);
int      redux_delta_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                                void *stream);
uint64_t redux_encode_delta_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_delta_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_delta_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                           void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                           void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                           void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_delta_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                           uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                           void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_delta(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                              uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                              uint32_t *block_crc);
int redux_decode_blocks_delta(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                              uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                              uint32_t *block_crc);

/* ---- zigzag-folded delta filter for signed series ----------------------------------------------
 * The delta filter's differences mod 2^(8E) put 0xFF into every upper byte when they are small and negative and 0x00 when
 * they are small and positive, so a series that moves both ways -- a sampled signal, a random walk, offsets that go back and
 * forth -- leaves each of the E - 1 upper byte planes an even mix of the two, about one bit per element per plane to a coder
 * that sees one plane per block.  These calls are the delta filter with every difference folded so that small magnitudes of
 * either sign become small unsigned numbers (Blosc, Parquet's DELTA_BINARY_PACKED and protobuf fold theirs the same way).
 * Strictly opt-in, as the delta filter is; monotone series lose nothing by it, and E = 1 gains nothing.  E, B and the frames
 * are the delta filter's.
 *   - d[0] = x[0] and d[i] = x[i] - x[i-1] mod 2^(8E), as for the delta filter.
 *   - z[i] = (d[i] << 1) ^ (0 - (d[i] >> (8E-1))) mod 2^(8E) for every i, 0 included: read as signed, d >= 0 maps to 2d and
 *     d < 0 to -2d - 1.  The L - N*E trailing bytes of a frame are unchanged.
 *   - The byte-plane layout above is then applied to the z's (E = 1: no layout).
 *   - The inverse undoes the layout, unfolds with d = (z >> 1) ^ (0 - (z & 1)) and takes the running sum mod 2^(8E) inside
 *     each frame.
 * The fold is a bijection on E-byte words, so any input round-trips.  Behind the transform is the plain adaptive coder:
 *     stream_zigzag_E(x)[b] == redux_encode_blocks(planes_E(zigzag_E(x)))[b].
 * Not available with the static-table models, stored blocks, a base, constant blocks, the mixed layouts, the `_v` calls and
 * redux_compress / redux_decompress.
 *
 * Every call is the shape of its delta namesake and keeps its promises: redux_zigzag_planes_dev is one read and one write;
 * redux_decode_zigzag_dev writes no byte outside d_out[0 .. out_len), for damaged streams too, and every frame whose blocks
 * are all OK holds the original bytes; the output of the host-pointer pair depends on neither the chunk size nor the
 * devices, and block_crc is over the ORIGINAL bytes.
 */
int      redux_zigzag_check(uint32_t element_size);
int      redux_zigzag_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                                 void *stream);
uint64_t redux_encode_zigzag_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_zigzag_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_zigzag_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_zigzag_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                            void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_zigzag(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                               uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                               uint32_t *block_crc);
int redux_decode_blocks_zigzag(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                               uint32_t *block_crc);

/* ---- lagged delta filter for interleaved channels and fixed-width records ----------------------
 * Both delta filters take the difference to the element directly before.  Where several series are interleaved -- stereo or
 * multi-channel PCM, IMU and ADC logs, (x, y, z) vertex arrays, RGB(A) pixels, row-major tables of fixed-width records --
 * that element belongs to another channel and the difference is larger than the value; the right predecessor sits S
 * elements back (TIFF's predictor, PNG's Sub filter with its bytes per pixel and FLAC's per-channel prediction are the same
 * idea).  These calls are the zigzag-folded delta filter with a lag S, 1 <= S <= REDUX_LAG_MAX.  Strictly opt-in: a wrong
 * lag costs bytes, and no call chooses one.  E, B and the frames are the delta filter's.
 *   - d[i] = x[i] for i < S, d[i] = x[i] - x[i-S] mod 2^(8E) for i >= S.
 *   - z[i] is the zigzag fold of d[i] (above), always: there is no unfolded form.  The L - N*E trailing bytes of a frame
 *     are unchanged.
 *   - The byte-plane layout is then applied to the z's (E = 1: no layout).
 *   - The inverse undoes the layout, unfolds, then x[i] = d[i] + x[i-S]: S independent running sums per frame.
 *   - Every frame starts afresh, so the blocks of different frames stay independent.  S >= N is legal: it folds every
 *     element and subtracts nothing.  S = 1 is the zigzag filter, byte for byte.
 * Behind the transform is the plain adaptive coder:
 *     stream_lag_E_S(x)[b] == redux_encode_blocks(planes_E(lag_E_S(x)))[b].
 * Not available where the zigzag filter is not.
 *
 * Every call is the shape of its zigzag namesake with `lag` after element_size, and keeps its promises:
 * redux_decode_lag_dev writes no byte outside d_out[0 .. out_len), for damaged streams too, and every frame whose blocks are
 * all OK holds the original bytes; the host-pointer pair cuts its chunks at frame boundaries, so its output depends on
 * neither the chunk size nor the devices, and block_crc is over the ORIGINAL bytes.  A lag of 0 or above REDUX_LAG_MAX is
 * REDUX_INVALID_INPUT wherever a bad element size is, and nothing is written.  The workspace calls take no lag and return
 * their zigzag namesakes' values.  redux_lag_planes_dev reads the source once from memory and once more from cache, and
 * reads no byte before a frame's first.
 */
#define REDUX_LAG_MAX 256
int      redux_lag_check(uint32_t element_size, uint32_t lag);
int      redux_lag_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, uint32_t lag,
                              int inverse, void *stream);
uint64_t redux_encode_lag_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_lag_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_lag_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                         uint32_t lag, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                         void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                         void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_lag_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                         uint32_t block_size, uint32_t element_size, uint32_t lag, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                         void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_lag(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                            uint32_t element_size, uint32_t lag, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                            int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_lag(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, uint32_t lag, uint8_t *out, uint32_t *out_sizes,
                            int32_t *block_status, uint32_t *block_crc);

/* ---- higher-order lagged differences -------------------------------------------------------------
 * The lagged delta filter predicts an element by the one S back, the weakest predictor that interleaved sampled data can
 * have.  A sampled, band-limited signal -- PCM, a vibration or IMU log, an ADC trace -- is locally a low-degree polynomial,
 * and the K-th difference removes one of degree K - 1: FLAC's fixed predictors of order 2 and 3, and every "delta of delta"
 * time-series codec.  These calls are the lagged delta filter applied K times, 1 <= K <= REDUX_LAG_ORDER_MAX.  Strictly
 * opt-in, as the lag is: on a random walk order 1 is already optimal and a higher order costs bytes (5 to 16 % on generated
 * walks, against a quarter to a third saved on generated tonal signals; no recorded signal was measured).  E, B, the frames
 * and the lag S are the lagged delta filter's.  With x[j] = 0 for j < 0:
 *   - d[i] = sum over j = 0 .. K of (-1)^j C(K, j) x[i - j S] mod 2^(8E):
 *       K = 2: x[i] - 2 x[i-S] + x[i-2S],  K = 3: x[i] - 3 x[i-S] + 3 x[i-2S] - x[i-3S].
 *     This is the lag-S difference applied K times, each application leaving its first S elements as they are.
 *   - z[i] is the zigzag fold of d[i], always.  The L - N*E trailing bytes of a frame are unchanged.
 *   - The byte-plane layout is then applied to the z's (E = 1: no layout).
 *   - The inverse undoes the layout, unfolds, then takes the S running sums of the frame K times.
 *   - Every frame starts afresh.  Any S and K are legal for any N: terms that fall before the frame are zero.  K = 1 is the
 *     lagged delta filter, byte for byte.
 * Behind the transform is the plain adaptive coder:
 *     stream_lag_order_E_S_K(x)[b] == redux_encode_blocks(planes_E(lag_order_E_S_K(x)))[b].
 * Not available where the lagged delta filter is not.
 *
 * Every call is the shape of its lag namesake with `order` directly after `lag`, and keeps its promises:
 * redux_decode_lag_order_dev writes no byte outside d_out[0 .. out_len), for damaged streams too, and every frame whose
 * blocks are all OK holds the original bytes; the host-pointer pair cuts its chunks at frame boundaries, and block_crc is
 * over the ORIGINAL bytes.  An order of 0 or above REDUX_LAG_ORDER_MAX is REDUX_INVALID_INPUT wherever a bad lag is, and
 * nothing is written; order 1 is accepted everywhere.  The workspace calls take neither lag nor order and return their zigzag
 * namesakes' values.  redux_lag_order_planes_dev reads the source once from memory and K times more from cache, and reads no
 * byte before a frame's first.
 */
#define REDUX_LAG_ORDER_MAX 3
int      redux_lag_order_check(uint32_t element_size, uint32_t lag, uint32_t order);
int      redux_lag_order_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size,
                                    uint32_t lag, uint32_t order, int inverse, void *stream);
uint64_t redux_encode_lag_order_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_lag_order_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_lag_order_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                               uint32_t lag, uint32_t order, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                               void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                               void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_lag_order_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint32_t lag, uint32_t order, void *d_out,
                               void *d_out_sizes /* u32[nblocks] */, void *d_block_status, void *d_summary, void *d_workspace,
                               uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_lag_order(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                  uint32_t element_size, uint32_t lag, uint32_t order, uint8_t *out, uint64_t out_cap,
                                  uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_lag_order(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                                  uint32_t block_size, uint32_t element_size, uint32_t lag, uint32_t order, uint8_t *out,
                                  uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- record layout for fixed-width structs ---------------------------------------------------------
 * A table of fixed-width records -- a packed C struct dump, a numpy structured array, a row-major page of a columnar store --
 * holds one distribution per byte column of the record.  The lag filter at element size 1 differences every byte against the
 * same byte of the record before, but leaves all R columns in the same blocks.  These calls are the byte-plane layout with a
 * record size R, 2 <= R <= REDUX_RECORD_MAX, in place of an element size (the HDF5 / Blosc "shuffle" with an arbitrary type
 * size), so that every block holds one byte column, with an optional byte delta against the record before.  Strictly opt-in;
 * adaptive model only.  B = block_size:
 *   - the input is cut into frames of R*B bytes, only the last may be shorter; a frame of L bytes holds N = L / R records;
 *   - delta != 0: d[i][p] = x[i][p] - x[i-1][p] mod 256 for i >= 1, d[0][p] = x[0][p]; every frame starts afresh; no fold
 *     (the adaptive model's cost of a block does not depend on a bijection of its byte values); delta == 0: d = x;
 *   - byte p of record i moves to frame offset p*N + i; the L - N*R trailing bytes stay where they are.
 *   Without the delta this is the byte-plane layout's rule with E = R, and for R = 2, 4, 8 redux_planes_dev's bytes.
 *     stream_record_R_F(x)[b] == redux_encode_blocks(record_R_F(x))[b].
 *
 * Every call is the shape of its lag namesake with (record_size, delta) in place of (element_size, lag), and keeps its
 * promises: redux_decode_record_dev writes no byte outside d_out[0 .. out_len), for damaged streams too, and every frame whose
 * blocks are intact decodes right; block_crc is over the ORIGINAL bytes.  A record size outside 2 .. REDUX_RECORD_MAX or a
 * delta other than 0 / 1 is REDUX_INVALID_INPUT, and nothing is written; the workspace calls take no delta, return 0 for such a
 * record size and otherwise what the lag family's return for element size 1.  redux_record_planes_dev: full frames go to
 * k_record_planes / k_record_unplanes when block_size, d_src and d_dst are multiples of 16, everything else (the short last
 * frame included) to k_record_planes_bytes / k_record_unplanes_bytes; d_src and d_dst must not overlap; no workspace.  The
 * host-pointer pair runs on the chunk pipeline with chunks rounded up to whole frames of R blocks; streams depend on neither
 * the chunk size nor the devices.
 * redux_host_chunk_plan_record   redux_host_chunk_plan for these calls: the chunk a multiple of record_size blocks.
 * redux_record_kernel_name       the kernels redux_record_planes_dev runs on 16-byte aligned buffers, joined by " + " when
 *                                full frames are followed by a short one; "" for arguments the call refuses.
 * redux_record_kernel_name_at    the same for these buffers, which contribute their alignment only.
 * redux_record_plan              the shape of that launch on 16-byte aligned buffers, from the function the launch itself
 *                                takes it from; nothing is launched.  plan: four values, plan[0] = lgT (the fast kernel's tile is 1 << lgT
 *                                records), plan[1] = PC (the inverse's byte columns per workgroup: record_size, or a multiple
 *                                of 16 that is at least 64), plan[2] = the fast kernel's grid, plan[3] = the byte kernel's
 *                                grid; a grid of 0: that kernel does not run.  cus: the CU count to plan for, 0 for the
 *                                current device's.  REDUX_INVALID_INPUT for arguments the call refuses. */
#define REDUX_RECORD_MAX 256
int      redux_record_check(uint32_t record_size, int delta);
int      redux_record_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t record_size, int delta,
                                 int inverse, void *stream);
uint64_t redux_encode_record_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t record_size);
uint64_t redux_decode_record_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t record_size);
int redux_encode_record_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t record_size,
                            int delta, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] or NULL */, void *d_workspace,
                            uint64_t workspace_bytes, void *stream);
int redux_decode_record_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                            uint32_t block_size, uint32_t record_size, int delta, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] or NULL */, void *d_workspace,
                            uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_record(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t record_size,
                               int delta, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                               uint32_t *block_crc);
int redux_decode_blocks_record(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t record_size, int delta, uint8_t *out, uint32_t *out_sizes,
                               int32_t *block_status, uint32_t *block_crc);
int redux_host_chunk_plan_record(uint64_t nblocks, uint32_t block_size, uint32_t record_size, uint32_t ncontexts, int decode,
                                 uint64_t *chunk_blocks, uint64_t *nchunks);
const char *redux_record_kernel_name(uint64_t len, uint32_t block_size, uint32_t record_size, int inverse);
const char *redux_record_kernel_name_at(const void *d_src, const void *d_dst, uint64_t len, uint32_t block_size,
                                        uint32_t record_size, int inverse);
int redux_record_plan(uint64_t len, uint32_t block_size, uint32_t record_size, int delta, int inverse, uint32_t cus,
                      uint32_t *plan);

/* ---- XOR-against-base filter for series of snapshots -------------------------------------------
 * A snapshot of tensors that were stored before -- checkpoint N against checkpoint N - 1, a fine-tuned model against its
 * base model, optimizer state, a KV cache against its earlier self -- differs from its predecessor only in the low mantissa
 * bits.  These calls take a second buffer, the BASE, and code the bytewise XOR against it: equal sign, exponent and high
 * mantissa bytes become zeros, which the adaptive coder writes in a fraction of a bit each.  XOR and not the modular
 * difference of the elements: a small negative difference puts 0xFF into every upper byte, and XOR needs no element
 * arithmetic.  Strictly opt-in, and only worth it when the base is related to the input; the decoder needs the same base.
 * E = element_size, one of 1, 2, 4, 8; B = block_size; x = the input, len bytes; y = the base, base_len bytes, any length.
 *   - y'[i] = y[i] for i < min(len, base_len) and 0 beyond: a base longer than the input is used up to len, a shorter one
 *     leaves the rest of x as it is.
 *   - d[i] = x[i] ^ y'[i] for every byte: no frames, no elements, the filter is bytewise.
 *   - The byte-plane layout above is then applied to d (E = 1: no layout).
 *   - The inverse undoes the layout and XORs with y' again.
 * Blocks and frames stay independent, x == y gives all-zero coder input, and a chunk boundary of the host calls changes
 * nothing (chunks are whole 64-block waves, so whole frames, and a chunk XORs its own share of the base).  Behind the
 * transform is the plain adaptive coder:
 *     stream_base_E(x, y)[b] == redux_encode_blocks(planes_E(x ^ y'))[b].
 * Not available with the static-table models, stored blocks, the delta filter, the `_v` calls and redux_compress /
 * redux_decompress.  Constant blocks (below) can be skipped behind it.
 *
 * redux_base_check          OK for 1, 2, 4, 8, else INVALID_INPUT.
 * redux_base_planes_dev     filter + layout (inverse = 0) or their inverse (inverse != 0) of len bytes, d_src -> d_dst, with
 *                           d_base[0 .. base_len) (null only with base_len 0).  d_dst must overlap neither d_src nor the
 *                           bytes of d_base that are read (INVALID_INPUT); stream-ordered, two reads and one write.
 * redux_encode_base_dev     redux_encode_blocks_dev of the transformed input, the transformed copy carved from the FRONT of
 *                           the workspace (redux_encode_base_workspace_bytes: for E = 1 too, the filter changes the bytes).
 * redux_decode_base_dev     redux_decode_planes_dev's procedure: the blocks decode into a plane buffer in the workspace, a
 *                           block that comes back OK with another size than its place gives it is reported INVALID_INPUT,
 *                           the inverse writes d_out[0 .. out_len) and no byte outside it, for damaged streams too.  Every
 *                           frame whose blocks are all OK holds the original bytes.
 * redux_encode_blocks_base  host-pointer forms on the chunk pipeline of redux_encode_blocks / redux_decode_blocks: base is
 * redux_decode_blocks_base  host memory, and a chunk's share of it travels to the device next to the chunk.  The output
 *                           depends on neither the chunk size nor the devices of redux_host_set_devices.  block_crc may be
 *                           null; else u32[nblocks], the CRC-32 of every block's ORIGINAL bytes, as for the delta filter.
 */
int      redux_base_check(uint32_t element_size);
int      redux_base_planes_dev(const void *d_src, const void *d_base, uint64_t base_len, void *d_dst, uint64_t len,
                               uint32_t block_size, uint32_t element_size, int inverse, void *stream);
uint64_t redux_encode_base_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_base_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_base_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                          uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap,
                          void *d_out_offsets /* u64[nblocks+1] */, void *d_block_status /* i32[nblocks] */,
                          void *d_summary /* i32[2] */, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_base_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                          const void *d_base, uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                          void *d_out, void *d_out_sizes /* u32[nblocks] */, void *d_block_status, void *d_summary,
                          void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_base(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                             uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                             int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_base(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                             uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                             uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- folded difference against a base ------------------------------------------------------------
 * A second operation for the base filter above, next to XOR and as opt-in as it is.  XOR is large where the input and the
 * base lie on opposite sides of a carry: 0x3F7FFFFF against 0x3F800000 differ by 1 and XOR to 0x00FFFFFF.  The difference
 * of the elements is small whenever the two are close as numbers, and the zigzag fold above takes away what spoke against
 * it, the 0xFF a small negative difference puts into every upper byte.  E, B, the frames and the byte-plane layout are as
 * above; x = the input, len bytes; y = the base, base_len bytes, any length; U = min(len, base_len), y'[i] = y[i] for i < U
 * and 0 beyond.
 *   - An element -- one of the N = L / E little-endian words of a frame of L bytes, counted from the frame's start -- is
 *     COVERED when all E of its bytes lie below U.  A covered element becomes z = (d << 1) ^ (0 - (d >> (8E-1))) mod 2^(8E)
 *     with d = x - y mod 2^(8E): read as signed, d >= 0 maps to 2d and d < 0 to -2d - 1.
 *   - Every other byte is x ^ y': an element the base ends inside, the L - N*E trailing bytes of a frame, everything past
 *     the base (which stays as it is).
 *   - The byte-plane layout is then applied (E = 1: no layout; the filter over single bytes, fold(x - y mod 256), remains).
 *   - The inverse undoes the layout, unfolds the covered elements with d = (z >> 1) ^ (0 - (z & 1)) and adds y; the other
 *     bytes are XORed with y' again.
 * x == y still gives all-zero coder input, whole frames past the base see the layout alone, and the rule is local to a frame
 * and to a prefix of the base: blocks and frames stay as independent as the layout leaves them, and a chunk of the host
 * calls works on its own share of the base.  The fold is a bijection, so any input round-trips.  Behind the transform is the
 * plain adaptive coder:
 *     stream_base_sub_E(x, y)[b] == redux_encode_blocks(planes_E(sub_E(x, y')))[b].
 * Not available with the static-table models, stored blocks, the delta filters, constant blocks, the mixed layouts, the `_v`
 * calls and redux_compress / redux_decompress.
 *
 * Every call has the signature of its base namesake and keeps its promises: redux_base_sub_planes_dev is two reads and one
 * write, and d_dst must overlap neither d_src nor the bytes of d_base that are read (INVALID_INPUT);
 * redux_decode_base_sub_dev writes no byte outside d_out[0 .. out_len), for damaged streams too, and every frame whose
 * blocks are all OK holds the original bytes; the output of the host-pointer pair depends on neither the chunk size nor the
 * devices, and block_crc is over the ORIGINAL bytes.  The workspaces are the base calls'.
 */
int      redux_base_sub_check(uint32_t element_size);
int      redux_base_sub_planes_dev(const void *d_src, const void *d_base, uint64_t base_len, void *d_dst, uint64_t len,
                                   uint32_t block_size, uint32_t element_size, int inverse, void *stream);
uint64_t redux_encode_base_sub_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_base_sub_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_base_sub_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                              uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap,
                              void *d_out_offsets /* u64[nblocks+1] */, void *d_block_status /* i32[nblocks] */,
                              void *d_summary /* i32[2] */, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_base_sub_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                              const void *d_base, uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                              void *d_out, void *d_out_sizes /* u32[nblocks] */, void *d_block_status, void *d_summary,
                              void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_base_sub(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                                 uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                 int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_base_sub(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                                 uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                                 uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- snapshot-stride filter for time series of fields ---------------------------------------------
 * One buffer of T snapshots of the same S elements -- a trajectory [frame, atom, xyz], a field [time, lat, lon], a stack of
 * sensor frames, a tensor logged every step -- predicts an element best by the same element one snapshot back: a distance of
 * thousands to millions of elements, out of REDUX_LAG_MAX's reach, and within the base filter's only by cutting the buffer
 * into T files.  These calls are the folded difference of the base filter with the second operand taken from the input
 * itself, S elements back.  Strictly opt-in: on unrelated snapshots it costs bytes, and no call chooses it.
 *   - E = element_size (1, 2, 4 or 8), B = block_size, S >= 1 the stride in elements (a u64), x = the input of len bytes,
 *     n = len / E whole little-endian elements counted from byte 0 of the WHOLE buffer, not per frame.
 *   - z[i] = x[i] for i < S; for S <= i < n: d = x[i] - x[i - S] mod 2^(8E), z[i] = (d << 1) ^ (0 - (d >> (8E - 1))), the fold
 *     of the zigzag filter.  The len - n*E trailing bytes are unchanged.  The byte-plane layout of E (frames of E*B bytes; none
 *     for E = 1) is applied to z.  S >= n is legal and is the layout alone.
 *   - The inverse undoes the layout; then, for i from S upward, x[i] = ((z[i] >> 1) ^ (0 - (z[i] & 1))) + x[i - S].
 *   - stream_stride_E_S(x)[b] == redux_encode_blocks(planes_E(stride_E_S(x)))[b].
 * This is the first filter whose predecessor lies outside the frame: the inverse of a block needs the blocks before it in its
 * columns.  So there are no range reads behind it, and the host-pointer pair does not run on the chunk pipeline: it stages
 * the WHOLE buffer on the first device of the host context (the current device, or the first of redux_host_set_devices) and
 * runs the _dev call there.  Its output therefore depends on neither the chunk size nor the devices, and block_crc is over the
 * ORIGINAL bytes; redux_host_chunk_plan does not describe it.
 *
 * Every call is the shape of its lag namesake with `stride`, a u64, where the lag is, except:
 *   - the inverse's second stage cuts time into segments where S is small (no launch holds a serial chain proportional to
 *     len) and keeps the segments' sums in a workspace: redux_stride_planes_dev takes (d_workspace, workspace_bytes) in front
 *     of the stream, at least redux_stride_workspace_bytes(len, element_size, stride) bytes for inverse != 0 (0: none needed;
 *     forward takes none, and null is fine then), REDUX_OUTPUT_TOO_SMALL with nothing written otherwise;
 *   - redux_decode_stride_workspace_bytes takes the stride too, for the same reason.
 * Bad arguments -- an element size outside {1, 2, 4, 8}, stride 0, overlapping d_src / d_dst -- are REDUX_INVALID_INPUT with
 * nothing written.  redux_decode_stride_dev writes no byte outside d_out[0 .. out_len), for damaged streams too; a block that
 * is not OK says so in its status, and the bytes at and after it in its columns are unspecified.  redux_stride_planes_dev
 * reads no byte before d_src.  redux_stride_kernel_name names what a transform call runs for these arguments and pointers
 * (their alignment counts; null: aligned), joined by " + ": "k_stride_planes", "k_stride_planes_bytes" forward; the layout's
 * inverse ("k_planes", "k_planes_bytes", "copy" for E = 1) and then "k_stride_sum", with "k_stride_totals" and
 * "k_stride_scan" in front of it where time is cut into segments, each with "_bytes" where a column is one element, and
 * "k_stride_sum_tail"; "" for arguments the call refuses and for len 0. */
int      redux_stride_check(uint32_t element_size, uint64_t stride);
uint64_t redux_stride_workspace_bytes(uint64_t len, uint32_t element_size, uint64_t stride);
int      redux_stride_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size,
                                 uint64_t stride, int inverse, void *d_workspace, uint64_t workspace_bytes, void *stream);
uint64_t redux_encode_stride_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_stride_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                                             uint64_t stride);
int redux_encode_stride_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint64_t stride, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] or NULL */, void *d_workspace,
                            uint64_t workspace_bytes, void *stream);
int redux_decode_stride_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, uint64_t stride, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                            void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] or NULL */, void *d_workspace,
                            uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_stride(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                               uint32_t element_size, uint64_t stride, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                               int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_stride(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint64_t stride, uint8_t *out, uint32_t *out_sizes,
                               int32_t *block_status, uint32_t *block_crc);
const char *redux_stride_kernel_name(uint64_t len, uint32_t block_size, uint32_t element_size, uint64_t stride, int inverse,
                                     const void *d_src, const void *d_dst);

/* ---- stored blocks -----------------------------------------------------------------------------
 * A block whose stream does not shrink it can travel as its raw bytes instead (zstd raw blocks, deflate stored blocks).
 * Block b has L_b = min(B, len - b*B) bytes of coder input x' (the input for element_size 1, its byte-plane layout for
 * E = 2, 4, 8: a stored plane is plane bytes) and a stream of s_b bytes.  With store_ratio t, 0 <= t <= 65536:
 *     stored_b  <=>  status_b == OK  and  s_b * 65536 >= t * L_b      (exact, 64-bit)
 * and payload_b = x'[b*B .. b*B + L_b) if stored_b, else the stream the plain / planes call writes, unchanged.  So
 * t = 65536 stores exactly the blocks that do not shrink (the output is never larger than the input plus its tables, and
 * costs no ratio on any input), t = 0 stores every block (an empty input's one block: a 0-byte payload).  t > 65536 is
 * INVALID_INPUT.  Flags are u8, 0 (coded) or 1 (stored), one per block.  Streams and flags depend on neither the chunk
 * size nor the devices.
 * Coverage: the adaptive model with symbol_bits 8 and code_bits <= 32 (the parameters of the `_v` calls); other valid
 * parameters are UNSUPPORTED.  Not available for the static-table model, the `_v` calls and redux_compress / decompress.
 *
 * redux_encode_stored_workspace_bytes  what redux_encode_stored_dev needs (the planes call's workspace); 0 if unsupported.
 * redux_decode_stored_workspace_bytes  what redux_decode_stored_dev needs for out_len bytes; 0 if unsupported.
 * redux_encode_stored_dev   the coder over x', then the rule (k_store_select): d_stored[b] is written, a stored block's
 *                           payload is x' itself and d_out_offsets counts its L_b bytes.  out_cap as in the plain call
 *                           (a block that does not fit is reported OUTPUT_TOO_SMALL and never written).
 * redux_decode_stored_dev   the inverse: nblocks = redux_block_count(out_len, B); out[0 .. out_len) in original order.  The
 *                           coded blocks decode through the table form of the adaptive decoders, the stored payloads are
 *                           copied.  Block b must come back as L_b bytes (for E > 1: its place in the frame layout): an OK
 *                           block of another length is INVALID_INPUT, a stored payload longer than L_b OUTPUT_TOO_SMALL
 *                           (size 0, nothing written), a flag other than 0 / 1 INVALID_INPUT.  d_summary (if given) is
 *                           overwritten with the failing blocks only.  out_cap must be >= out_len.
 * redux_encode_blocks_stored / redux_decode_blocks_stored  host-pointer forms through the chunk pipeline; the flags
 *                           travel per chunk as the CRCs do (block_crc may be NULL, as in the `_crc` calls). */
uint64_t redux_encode_stored_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_stored_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_stored_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint32_t store_ratio, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                            void *d_stored /* u8[nblocks] */, void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_decode_stored_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                            const void *d_stored /* u8[nblocks] */, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                            void *d_out, uint64_t out_cap, void *d_out_sizes /* u32[nblocks] */, void *d_block_status,
                            void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_stored(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                               uint32_t store_ratio, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, uint8_t *stored,
                               int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_stored(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *stored,
                               uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap,
                               uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- constant blocks ---------------------------------------------------------------------------
 * A block whose bytes are all equal can travel as that one byte and skip the coder in both directions: behind the
 * XOR-against-base filter every unchanged region of a snapshot is such a block, which the coder would still write in
 * about 300 bytes per 64 KiB and at coder rate.  Strictly opt-in; stored blocks handle the incompressible end, this the
 * other one.  x' is the coder input: the input itself for element_size 1, its byte-plane layout for E = 2, 4, 8, or the
 * layout of x ^ base' when a base is given (the XOR-against-base filter above; base_len 0 means no base, d_base / base may
 * then be null).  Block b has L_b = min(B, len - b*B) bytes of x'.
 *     const_b  <=>  L_b >= 1  and  all L_b bytes of block b are equal      (a 1-byte block is constant; the empty
 *                                                                           input's one empty block is not)
 *   - If const_b, payload_b is that one byte and the size entry is 1.
 *   - Otherwise payload_b is the stream the plain, planes or base call writes for block b, bit for bit.
 *   - Flags are u8, 0 (coded) or 1 (constant), one per block.
 *   - Streams and flags depend on neither the chunk size nor the devices.
 * Coverage: the adaptive model with symbol_bits 8 and code_bits <= 32, as for stored blocks (other valid parameters are
 * UNSUPPORTED); any element_size of 1, 2, 4, 8; with or without a base; with or without per-block CRCs (of the ORIGINAL
 * bytes, as for the base calls).  Not available with stored blocks, the delta filter, the static-table models, the `_v`
 * calls and redux_compress / redux_decompress.
 *
 * redux_const_blocks_dev    the detection alone (k_const_select) over any buffer: d_flags[b] for the nblocks =
 *                           redux_block_count(in_len, B) blocks of d_in; one read of the buffer at most (a block is left at
 *                           the first difference found), any alignment, stream-ordered.
 * redux_encode_const_workspace_bytes  what redux_encode_const_dev needs, with or without a base; 0 if unsupported.
 * redux_decode_const_workspace_bytes  what redux_decode_const_dev needs for out_len bytes; 0 if unsupported.
 * redux_encode_const_dev    x' at the front of the workspace, the detection (d_const[b] is written), then the table form of
 *                           the coder over the blocks that are left; a constant block gets size 1 and status OK, and its
 *                           byte is copied from x'.  out_cap as in the plain call.  The table encoder's limit applies: an
 *                           input of 4 GiB or more is UNSUPPORTED (the host-pointer form chunks far below it).
 * redux_decode_const_dev    the inverse: nblocks = redux_block_count(out_len, B); d_out[0 .. out_len) in original order and
 *                           no byte outside it.  The coded blocks decode through the table form of the adaptive decoders,
 *                           a constant block is a fill of its L_b bytes.  d_const is untrusted: a flag other than 0 / 1, a
 *                           constant block whose payload is not exactly 1 byte and a constant flag on a block with L_b = 0
 *                           are INVALID_INPUT for that block (size 0, nothing written); an OK block of another length than
 *                           its place is INVALID_INPUT as in the planes call.  d_summary (if given) is overwritten with
 *                           the failing blocks only.
 * redux_encode_blocks_const / redux_decode_blocks_const  host-pointer forms on the chunk pipeline; the flags travel per
 *                           chunk as the stored flags do, a chunk's share of the base as in the base calls.  block_crc may
 *                           be NULL. */
int      redux_const_blocks_dev(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_flags /* u8[nblocks] */, void *stream);
uint64_t redux_encode_const_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_decode_const_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int redux_encode_const_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                           uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap,
                           void *d_out_offsets /* u64[nblocks+1] */, void *d_const /* u8[nblocks] */,
                           void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */, void *d_workspace,
                           uint64_t workspace_bytes, void *stream);
int redux_decode_const_dev(const redux_params *p, const void *d_in, const void *d_in_offsets /* u64[nblocks+1] */,
                           const void *d_const /* u8[nblocks] */, const void *d_base, uint64_t base_len, uint64_t out_len,
                           uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes /* u32[nblocks] */,
                           void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int redux_encode_blocks_const(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                              uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                              uint8_t *const_flags, int32_t *block_status, uint32_t *block_crc);
int redux_decode_blocks_const(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *const_flags,
                              const uint8_t *base, uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                              uint8_t *out, uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- per-block CRC-32 checksums ---------------------------------------------------------------
 * crc[b] = CRC-32/ISO-HDLC -- the zlib / gzip / PNG CRC (reflected polynomial 0xEDB88320, init and xorout 0xFFFFFFFF),
 * zlib.crc32 -- of the ORIGINAL, uncompressed bytes x[b*B .. min((b+1)*B, len)), B = block_size.  The same for every model
 * and layout: with the byte-plane layout block b of the checksum is an original-order range, not plane b.  An empty input
 * is one empty block with CRC 0.  Computed on the device (k_crc32, redux_amd/csrc/redux_crc.hpp) from the linearity of the
 * CRC over GF(2): the terms of a block's pieces are combined by XOR in any order.  Any block size, any alignment.
 *
 * redux_crc32_blocks_dev    crc[b] of d_in[0 .. in_len) in blocks of block_size: redux_block_count(in_len, block_size)
 *                           entries in d_crc (u32, device).  Stream-ordered, never allocates, never synchronises.
 * redux_crc32_sizes_dev     the layout redux_decode_blocks_dev writes: block b = d_in[b*B .. b*B + min(sizes[b], B)),
 *                           d_sizes u32[nblocks] on the device.
 * redux_crc32_combine       zlib's crc32_combine, on the host: the CRC of A || B from crc(A), crc(B) and |B| (a whole file's
 *                           CRC from its block CRCs).
 * redux_crc32_blocks        host pointers: chunks staged through the host pipeline's pinned ring on the CURRENT device (as
 *                           redux_static_table; redux_host_set_devices is ignored), crc[] in host memory.
 * The `_crc` coding calls take their sibling's arguments plus block_crc (u32[nblocks], host memory):
 *   - encode: crc[b] of the input, computed on each chunk's staged input in HBM before any transform;
 *   - decode: the CRC of what block b decoded to (planes: the original-order range after the inverse transform), computed
 *     on each chunk's output in HBM; unspecified for a block whose status is not OK.
 * Their CRCs cost no extra PCIe traffic (4 bytes per block travel with the chunk's other small arrays) and depend on
 * neither the chunk size nor the devices.  The sibling calls are these with block_crc = NULL.  A caller that finds a
 * mismatch reports INVALID_INPUT (there is no status code of its own). */
int      redux_crc32_blocks_dev(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_crc /* u32[nblocks] */, void *stream);
int      redux_crc32_sizes_dev(const void *d_in, uint64_t nblocks, uint32_t block_size, const void *d_sizes /* u32[nblocks] */,
                               void *d_crc /* u32[nblocks] */, void *stream);
uint32_t redux_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
int      redux_crc32_blocks(const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t *crc);
int      redux_encode_blocks_crc(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint8_t *out,
                                 uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc);
int      redux_decode_blocks_crc(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks,
                                 uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes, int32_t *block_status,
                                 uint32_t *block_crc);
int      redux_encode_blocks_planes_crc(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                        uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                        int32_t *block_status, uint32_t *block_crc);
int      redux_decode_blocks_planes_crc(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                                        uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes,
                                        int32_t *block_status, uint32_t *block_crc);
int      redux_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                        uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                        int32_t *block_status, uint32_t *block_crc);
int      redux_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in,
                                        const uint64_t *in_offsets, uint64_t nblocks, uint32_t block_size, uint8_t *out,
                                        uint64_t out_cap, uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- plane-static coding: one static table per byte plane ----------------------------------------
 * The byte-plane layout and the semi-static model together: typed data (bf16 / fp32 / int64) whose planes have very different
 * statistics, coded by the static coder under a table per plane.  E = element_size, one of 1, 2, 4, 8; B = block_size;
 * x' = the byte-plane layout of the input for E and B ("byte-plane layout" above; E = 1: the input itself); block b of x' is
 * x'[b*B .. min((b+1)*B, len)).
 * The rule:
 *   1. Table t, 0 <= t < E, is the table of "semi-static coding" (redux_static_table_from_counts) of the counts of the bytes
 *      of all blocks b of x' with b mod E == t.  For full frames that is plane t; the short last frame is not special-cased:
 *      its blocks are counted, and coded, by their index like any other.  A t that owns no bytes (len <= t*B) gets the table
 *      of N = 0: every frequency 1, total 257.
 *   2. Block b is coded under table b mod E by the static coder:
 *      stream[b] == redux_static_encode_blocks(block b of x', cum[b mod E]); E = 1 is the static-table model, stream for stream.
 *   3. Every table has the same total (one `total` argument), so one launch runs one kernel instance; the table of a t that
 *      owns no bytes keeps total 257, and the only block ever coded under one is the empty input's block 0.
 * Tables are u32[E][258], table t at cum + 258 t.  On the device they are read from device memory (d_cum), and the kernels
 * check the table they load: one that is not strictly increasing from 0 to `total` (or to 257) makes its blocks INVALID_INPUT.
 * Not available for the `_v` calls, redux_compress / redux_decompress and stored blocks; one set of tables per call (tables
 * per block range: "segment-static coding" below).
 *
 * redux_plane_static_table_check        every table passes redux_static_table_check, and all totals are equal (a table of
 *                                       total 257, what a t without bytes gets, goes with any).  E = 1: one table.
 * redux_plane_static_total              the common total of checked tables (the largest cum[257]).
 * redux_plane_static_tables_from_counts rule 1 on the host from u64[E][256] counts.
 * redux_plane_histogram_dev             ADDS the counts of x' = d_in[0 .. in_len) (already in the layout) to d_counts,
 *                                       u64[E][256]: block b's bytes go to table b mod E.  Any block size and alignment.  A
 *                                       buffer can be counted in pieces that are whole frames of E*B bytes.  Workspace: none.
 * redux_plane_static_tables_dev         redux_static_table_dev for each t: d_counts + 256 t -> d_cum + 258 t.
 * redux_plane_static_tables             host pointers, input in ORIGINAL order: chunks of whole frames are staged through the
 *                                       pinned ring on the current device (as redux_static_table), laid out and counted there.
 * redux_plane_static_encode_dev         device pointers, input in original order: the layout into the front of the workspace,
 * redux_plane_static_decode_dev         then rule 2; decode is redux_decode_planes_dev's procedure under the static decoders
 *                                       (plane buffer in the workspace, an OK block of the wrong length is INVALID_INPUT,
 *                                       nothing outside d_out[0 .. out_len) is written, the summary last).  E = 1: no copy.
 * redux_plane_static_encode_blocks_crc  host pointers through the chunk pipeline (fleet included), block_crc nullable: the
 * redux_plane_static_decode_blocks_crc  CRCs are those of the ORIGINAL bytes, as for every layout.  The streams depend on
 *                                       neither the chunk size nor the devices. */
int      redux_plane_static_table_check(const redux_params *p, const uint32_t *cum /* u32[E][258] */, uint32_t element_size);
uint32_t redux_plane_static_total(const uint32_t *cum, uint32_t element_size);
int      redux_plane_static_tables_from_counts(const redux_params *p, const uint64_t *counts /* u64[E][256] */, uint32_t element_size,
                                               uint32_t total, uint32_t *cum);
uint64_t redux_plane_histogram_workspace_bytes(uint64_t in_len);
int      redux_plane_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                                   void *d_counts /* u64[E][256], ADDED to */, void *d_workspace, uint64_t workspace_bytes, void *stream);
int      redux_plane_static_tables_dev(const redux_params *p, const void *d_counts, uint32_t element_size, uint32_t total,
                                       void *d_cum /* u32[E][258] */, void *stream);
int      redux_plane_static_tables(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                                   uint32_t total, uint32_t *cum);
uint64_t redux_plane_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_plane_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_plane_static_decode_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
int      redux_plane_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                       uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap,
                                       void *d_out_offsets /* u64[nblocks+1] */, void *d_block_status /* i32[nblocks] */,
                                       void *d_summary /* i32[2] */, void *d_workspace, uint64_t workspace_bytes, void *stream);
int      redux_plane_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in,
                                       const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len, uint32_t block_size,
                                       uint32_t element_size, void *d_out, void *d_out_sizes /* u32[nblocks] */, void *d_block_status,
                                       void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int      redux_plane_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                              uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap,
                                              uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc);
int      redux_plane_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, const uint64_t *in_offsets,
                                              uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                                              uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- segment-static coding: static tables per block range ------------------------------------------
 * Plane-static coding with tables that follow the data: one table (or E, one per byte plane) covers a whole input, and loses
 * where the statistics move (a checkpoint is a concatenation of tensors with different scales).  E = element_size, one of
 * 1, 2, 4, 8; B = block_size; x' = the byte-plane layout of the input for E and B (E = 1: the input itself).
 * The rule:
 *   1. A segment is G = segment_blocks = 64 E k consecutive blocks of x', k >= 1 (G == 0 or not a multiple of 64 E:
 *      INVALID_INPUT).  Segment s holds blocks [s G, (s+1) G); nseg = max(1, ceil(nblocks / G)).
 *   2. Table (s, t), 0 <= t < E, is the table of "semi-static coding" (redux_static_table_from_counts, unchanged, one `total`
 *      for the whole call) of the counts of the bytes of all blocks b of segment s with b mod E == t.  A pair (s, t) that owns
 *      no bytes keeps the all-ones table (total 257), as in plane-static; the short last frame is not special-cased.
 *   3. Block b is coded by the static coder under table (b / G) E + b mod E:
 *      stream[b] == redux_static_encode_blocks(block b of x', cum[(b / G) E + b mod E]).
 *   4. With G >= nblocks the tables and streams are those of plane-static coding (E > 1) or of the static-table model
 *      (E = 1), bit for bit.
 * Tables are u32[nseg][E][258], counts u64[nseg][E][256]: table (s, t) at cum + 258 (s E + t).  The kernels check the table
 * they load, as in plane-static: a bad table makes only the blocks of the workgroup that loaded it INVALID_INPUT.  8-bit
 * symbols and code_bits <= 32, as for plane-static; everything else is UNSUPPORTED.  Not available for the `_v` calls,
 * redux_compress / redux_decompress and stored blocks.  Callers above the C ABI default to G = 64 E * 4.
 *
 * redux_segment_static_table_count        nseg E for nblocks blocks; 0 for an element size or G the rule does not take.
 * redux_segment_static_table_check        ntables == redux_segment_static_table_count(nblocks, ...), every table passes
 *                                         redux_static_table_check, and all totals are equal (a table of total 257 goes with any).
 * redux_segment_static_total              the common total of checked tables (the largest cum[257]).
 * redux_segment_static_tables_from_counts rule 2 on the host from u64[nseg][E][256] counts.
 * redux_segment_histogram_dev             ADDS the counts of x' = d_in[0 .. in_len) (already in the layout) to d_counts,
 *                                         u64[nseg][E][256] (k_segment_hist).  Any block size and alignment.
 * redux_segment_static_tables_dev         rule 2 on the device, one launch for all tables (k_static_tables).
 * redux_segment_static_encode_dev         device pointers, input in original order, as redux_plane_static_encode_dev /
 * redux_segment_static_decode_dev         redux_plane_static_decode_dev with rule 3.
 * redux_segment_static_build_encode_dev   the tables built from the buffer they code: the layout once, the histogram of that
 *                                         copy, the tables (left in d_cum, u32[nseg][E][258]), the coder over the same copy.
 *                                         Workspace: redux_segment_static_build_encode_workspace_bytes.
 * redux_segment_static_encode_blocks_crc  host pointers through the chunk pipeline (fleet included), block_crc nullable.
 * redux_segment_static_decode_blocks_crc  Chunks are whole segments; encode builds each chunk's tables from that chunk (one
 *                                         pass over the input: no histogram of the whole input first) and writes them to cum,
 *                                         u32[redux_segment_static_table_count][258] in host memory; decode sends each chunk
 *                                         its own tables.  Streams and tables depend on neither the chunk size nor the devices. */
uint64_t redux_segment_static_table_count(uint64_t nblocks, uint32_t element_size, uint32_t segment_blocks);
int      redux_segment_static_table_check(const redux_params *p, const uint32_t *cum, uint64_t ntables, uint64_t nblocks,
                                          uint32_t element_size, uint32_t segment_blocks);
uint32_t redux_segment_static_total(const uint32_t *cum, uint64_t ntables);
int      redux_segment_static_tables_from_counts(const redux_params *p, const uint64_t *counts, uint64_t nblocks, uint32_t element_size,
                                                 uint32_t segment_blocks, uint32_t total, uint32_t *cum);
int      redux_segment_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                                     uint32_t segment_blocks, void *d_counts /* u64[nseg][E][256], ADDED to */, void *stream);
int      redux_segment_static_tables_dev(const redux_params *p, const void *d_counts, uint64_t nblocks, uint32_t element_size,
                                         uint32_t segment_blocks, uint32_t total, void *d_cum /* u32[nseg][E][258] */, void *stream);
uint64_t redux_segment_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_segment_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_segment_static_decode_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size);
uint64_t redux_segment_static_build_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size,
                                                           uint32_t element_size, uint32_t segment_blocks);
int      redux_segment_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                         uint32_t block_size, uint32_t element_size, uint32_t segment_blocks, void *d_out,
                                         uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                                         void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */, void *d_workspace,
                                         uint64_t workspace_bytes, void *stream);
int      redux_segment_static_build_encode_dev(const redux_params *p, uint32_t total, const void *d_in, uint64_t in_len,
                                               uint32_t block_size, uint32_t element_size, uint32_t segment_blocks,
                                               void *d_cum /* u32[nseg][E][258], written */, void *d_out, uint64_t out_cap,
                                               void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                                               uint64_t workspace_bytes, void *stream);
int      redux_segment_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in,
                                         const void *d_in_offsets /* u64[nblocks+1] */, uint64_t out_len, uint32_t block_size,
                                         uint32_t element_size, uint32_t segment_blocks, void *d_out,
                                         void *d_out_sizes /* u32[nblocks] */, void *d_block_status, void *d_summary,
                                         void *d_workspace, uint64_t workspace_bytes, void *stream);
int      redux_segment_static_encode_blocks_crc(const redux_params *p, uint32_t total, const uint8_t *in, uint64_t in_len,
                                                uint32_t block_size, uint32_t element_size, uint32_t segment_blocks,
                                                uint32_t *cum /* written */, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                                int32_t *block_status, uint32_t *block_crc);
int      redux_segment_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, uint64_t ntables, const uint8_t *in,
                                                const uint64_t *in_offsets, uint64_t out_len, uint32_t block_size,
                                                uint32_t element_size, uint32_t segment_blocks, uint8_t *out, uint32_t *out_sizes,
                                                int32_t *block_status, uint32_t *block_crc);

/* ---- context-static coding: a static table per preceding byte ----------------------------------------
 * The static models above code a byte under a distribution that ignores the byte before it.  Here the table depends on the
 * previous byte (an order-1 model): on text, logs and source code that is worth 20 % and more from about half a megabyte
 * upward; below that the 256 tables cost more than they save.  Strictly opt-in.  8-bit symbols and code_bits <= 32;
 * everything else is UNSUPPORTED.  B = block_size.
 * The rule:
 *   1. The context of byte i of a block is byte i-1 of the same block; the first byte of every block has context 0.  The EOF
 *      symbol is coded under the context of the block's last byte (0 for an empty block).  Blocks stay independent.
 *   2. counts[c][s], u64[256][256]: over all blocks, the number of bytes s whose context is c.  The pair across a block
 *      boundary is not counted; each block's first byte counts under c = 0.
 *   3. Table c is redux_static_table_from_counts(counts[c], total), unchanged, but for a context that owns no bytes: that one
 *      is given a count of one for every byte value before the rule is applied.  EVERY table therefore has the same total,
 *      and one reciprocal serves a launch.  (Plane-static's all-ones, total-257 table would not do: a caller may code data
 *      under tables built from other data, and any context can then occur.)
 *   4. total <= 2^16 and <= freq_max; a larger total is UNSUPPORTED, a smaller one than 257 INVALID_INPUT as for every static
 *      table.  So every cum[1..256] fits 16 bits, 256 tables are exactly 128 KiB on the device, and the coder's quotient
 *      needs no fix-up.
 *   5. Block b's stream is what Codec::compress_stream writes with a model whose get_frequency(s) answers from table ctx and
 *      then sets ctx = s; decode is the mirror through get_symbol.
 *   6. Tables are u32[256][258], table c at cum + 258 c, each in the format of every other static call.
 * On the device the tables are read from device memory (d_cum).  Every coder launch first checks them (strictly increasing
 * from 0 to `total`, all 256): if one fails, every block is INVALID_INPUT and nothing else is written.
 * Not available for the `_v` calls, redux_compress / redux_decompress, layouts, filters and stored blocks.
 *
 * redux_context_static_table_check        all 256 tables pass redux_static_table_check, and their totals are equal and <= 2^16.
 * redux_context_static_total              the total of checked tables (cum[257]).
 * redux_context_static_tables_from_counts rules 3 and 4 on the host from u64[256][256] counts.
 * redux_context_histogram_dev             ADDS the pair counts of d_in[0 .. in_len), cut into blocks of block_size from its
 *                                         start, to d_counts (u64[256][256]).  Any block size and alignment; a buffer can be
 *                                         counted in pieces that are whole blocks.
 * redux_context_static_tables_dev         rule 3 on the device, one launch for all 256: d_counts -> d_cum (u32[256][258]).
 * redux_context_static_tables             host pointers: chunks of whole blocks are staged through the pinned ring on the
 *                                         current device (as redux_static_table) and counted there.
 * redux_context_static_encode_dev         device pointers, the procedure of redux_static_encode_blocks_dev /
 * redux_context_static_decode_dev         redux_static_decode_blocks_dev (block b decodes to d_out + b*block_size; the summary
 *                                         last; nothing outside the output is written) with the tables in device memory and a
 *                                         workspace (256-byte aligned) that holds their checked image.
 * redux_context_static_encode_blocks_crc  host pointers through the chunk pipeline (fleet included), one set of tables per
 * redux_context_static_decode_blocks_crc  call, block_crc nullable.  Streams depend on neither the chunk size nor the devices. */
int      redux_context_static_table_check(const redux_params *p, const uint32_t *cum /* u32[256][258] */);
uint32_t redux_context_static_total(const uint32_t *cum);
int      redux_context_static_tables_from_counts(const redux_params *p, const uint64_t *counts /* u64[256][256] */, uint32_t total,
                                                 uint32_t *cum);
int      redux_context_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size,
                                     void *d_counts /* u64[256][256], ADDED to */, void *stream);
int      redux_context_static_tables_dev(const redux_params *p, const void *d_counts, uint32_t total, void *d_cum /* u32[256][258] */,
                                         void *stream);
int      redux_context_static_tables(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t total,
                                     uint32_t *cum);
uint64_t redux_context_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_context_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t redux_context_static_decode_workspace_bytes(const redux_params *p, uint64_t nblocks, uint32_t block_size);
int      redux_context_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                         uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_offsets /* u64[nblocks+1] */,
                                         void *d_block_status /* i32[nblocks] */, void *d_summary /* i32[2] */, void *d_workspace,
                                         uint64_t workspace_bytes, void *stream);
int      redux_context_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in,
                                         const void *d_in_offsets /* u64[nblocks+1] */, uint64_t nblocks, uint32_t block_size,
                                         void *d_out, uint64_t out_cap, void *d_out_sizes /* u32[nblocks] */, void *d_block_status,
                                         void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream);
int      redux_context_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                                uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                                int32_t *block_status, uint32_t *block_crc);
int      redux_context_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in,
                                                const uint64_t *in_offsets, uint64_t nblocks, uint32_t block_size, uint8_t *out,
                                                uint64_t out_cap, uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);

/* ---- size estimates --------------------------------------------------------------------------------------
 * What a block would cost under a model, from counts alone: every model here is exchangeable inside a block, so a block's
 * ideal code length is a function of its byte counts, not of the order of its bytes.  A caller compares models without
 * coding the input once per model.  Costs are in BITS, as doubles, and cross this boundary through pointers only.
 *   - Adaptive model (8-bit symbols): a block starts at total 257 and every coded symbol adds 1, so a block with histogram h
 *     and n bytes costs, the EOF symbol included,
 *         A(h, n) = log2 G(n + 258) - log2 G(257) - sum_s log2 G(h[s] + 1)                    (G = the gamma function).
 *     This holds while the model cannot freeze inside the block: 256 + n < freq_max.  A frozen model's cost depends on the
 *     order of the bytes, so a longer block is UNSUPPORTED, as are symbol_bits != 8 and code_bits > 32.
 *   - Static table cum[0..=257] with T = cum[257]: counts c cost sum_s c[s] (log2 T - log2(cum[s+1] - cum[s])), the
 *     cross-entropy of the counts under the table.  Terms with c[s] == 0 are 0; the result is +inf when T == 0, or when a
 *     frequency that is zero or negative meets a nonzero count.  EOF is NOT included: every table the library builds gives
 *     EOF frequency 1, so a caller adds log2 T per block.  Nothing is indexed by table contents: any bytes may be passed.
 *   - A stream is its ideal length plus the coder's termination: measured against the reference coder at (8, 30, 32),
 *     len(stream) - (ceil(A / 8) + 2) lies in -1 .. +1 for the adaptive model and len(stream) - bits / 8 in 1.78 .. 2.87 for
 *     static tables of total 2^16.
 *
 * redux_adaptive_cost_from_counts  A for n count rows, u64[n][256] -> bits[n], on the host; needs no GPU.  UNSUPPORTED
 *                                  unless symbol_bits == 8, code_bits <= 32 and 256 + the largest row sum < freq_max.
 * redux_table_cost_from_counts     the table rule for n rows, counts u64[n][256] and tables u32[n][258] -> bits[n], on the host.
 * redux_block_cost_dev             A for every block of d_in[0 .. in_len) cut into blocks of block_size from its start
 *                                  (k_block_cost): d_bits is f64[redux_block_count(in_len, block_size)] on the device.  Any
 *                                  block_size 1 .. 2^30 (else INVALID_INPUT), any alignment of d_in, a short last block,
 *                                  in_len == 0 (one empty block).  The UNSUPPORTED conditions above with block_size in
 *                                  place of the row sum.  Stream-ordered, no workspace.
 * redux_table_cost_dev             the table rule on the device (k_table_cost): d_counts u64[n][256] -- n = 1 what
 *                                  redux_histogram_dev leaves, E rows redux_plane_histogram_dev, nseg E
 *                                  redux_segment_histogram_dev, 256 redux_context_histogram_dev -- and d_cum u32[n][258]
 *                                  -> d_bits f64[n].  Stream-ordered, no workspace. */
int redux_adaptive_cost_from_counts(const redux_params *p, const uint64_t *counts /* u64[n][256] */, uint64_t n, double *bits);
int redux_table_cost_from_counts(const uint64_t *counts /* u64[n][256] */, const uint32_t *cum /* u32[n][258] */, uint64_t n,
                                 double *bits);
int redux_block_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                         void *d_bits /* f64[nblocks] */, void *stream);
int redux_table_cost_dev(const void *d_counts /* u64[n][256] */, const void *d_cum /* u32[n][258] */, uint64_t n,
                         void *d_bits /* f64[n] */, void *stream);

/* ---- layout estimates ------------------------------------------------------------------------------------
 * The adaptive cost A (above) of every block of the input under each of the eight layouts a caller can put in front of the
 * adaptive coder, so that the element size and the filter can be chosen without transforming or coding the input once per
 * candidate.  Layout k = 4 F + log2 E: the byte-plane layout for elements of E = 1, 2, 4, 8 bytes ("byte-plane layout"
 * above; E = 1: the bytes as they are), behind the delta filter when F = 1 ("delta filter" above; k = 4 is the filter over
 * single bytes).  Every transformed input has the input's length, so all eight have redux_block_count(in_len, block_size)
 * blocks.  Nothing about the layouts is new: bits[k][b] is what redux_block_cost_dev gives for block b of what
 * redux_planes_dev / redux_delta_planes_dev write for (E, F) -- short last frame, trailing bytes and fresh starts of the
 * frames included -- but it is counted from the untransformed bytes: no transformed copy, no workspace, and one read of
 * the input per element size (the plain and the delta counts of a frame are taken by two waves of one workgroup).
 *
 * redux_layout_cost_dev             d_bits is f64[8][nblocks] on the device; row k is written only when bit k of `layouts`
 *                                   is set.  Full frames go to k_layout_cost when block_size and d_in are multiples of 16,
 *                                   everything else (the short last frame included) to k_layout_cost_bytes, which is right
 *                                   for any alignment and block size but slow.  INVALID_INPUT for a block_size outside
 *                                   1 .. 2^30, layouts == 0 or a bit above 7; UNSUPPORTED as redux_block_cost_dev.
 *                                   in_len == 0: one empty block per row.  Stream-ordered, no workspace.
 * redux_layout_cost_kernel_name     the kernels layout k (0 .. 7) of such a call runs on a 16-byte aligned d_in:
 *                                   "k_layout_cost<E>", "k_layout_cost_bytes<E>", or both joined by " + " when full frames are
 *                                   followed by a short one.  "" for a block_size or layout out of range.
 * redux_layout_cost_kernel_name_at  the same for this d_in, which contributes its alignment only. */
int         redux_layout_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                                  uint32_t layouts /* bit k = layout k */, void *d_bits /* f64[8][nblocks] */, void *stream);
const char *redux_layout_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t layout);
const char *redux_layout_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t layout);

/* ---- lag estimates ---------------------------------------------------------------------------------------
 * The adaptive cost A (above) of every block of the input behind the lagged delta filter ("lagged delta filter" above), for a
 * list of lags in one call, so that the lag can be counted instead of known in advance or found by coding the input once per
 * candidate.  Nothing about the filter is new: bits[j][b] is what redux_block_cost_dev gives for block b of what
 * redux_lag_planes_dev writes for (element_size, block_size, lags[j]) -- the fresh start of every frame, d[i] = x[i] for
 * i < S, the fold, S >= N, the short last frame and its trailing bytes included -- but it is counted from the untransformed
 * bytes: no transformed copy and no workspace.
 *
 * Frame sampling.  With frame_step T only the frames 0, T, 2T, ... (of element_size * block_size bytes) are costed, and the
 * output is compact: row j holds the blocks of the selected frames in order.  A selected full frame contributes
 * element_size blocks, a selected short last frame the blocks it has.  T = 1 costs every block.
 *
 * redux_lag_cost_block_count     the blocks of a row: redux_block_count(in_len, block_size) for frame_step 1; 0 for a
 *                                block_size or frame_step of 0 or an element size that is not 1, 2, 4, 8.
 * redux_lag_cost_dev             d_bits is f64[nlags][redux_lag_cost_block_count(...)] on the device.  lags: nlags values on
 *                                the HOST, consumed before the call returns (they travel in the kernels' arguments); repeated
 *                                lags are legal, rows are independent.  Full frames go to k_lag_cost when block_size and d_in
 *                                are multiples of 16, everything else (the short last frame included) to k_lag_cost_bytes,
 *                                which is right for any alignment and block size but slow.  INVALID_INPUT for a block_size
 *                                outside 1 .. 2^30, an element size other than 1, 2, 4, 8, nlags == 0 or above
 *                                REDUX_LAG_MAX, a lag redux_lag_check refuses, frame_step == 0, or a null lags / d_bits;
 *                                UNSUPPORTED as redux_block_cost_dev.  in_len == 0: one empty block per row.
 *                                Stream-ordered, no workspace, no host synchronisation.
 * redux_lag_cost_kernel_name     the kernels such a call with frame_step 1 runs on a 16-byte aligned d_in: "k_lag_cost<E>",
 *                                "k_lag_cost_bytes<E>", or both joined by " + " when full frames are followed by a short
 *                                one.  "" for a block_size or element size out of range.
 * redux_lag_cost_kernel_name_at  the same for this d_in, which contributes its alignment only. */
uint64_t    redux_lag_cost_block_count(uint64_t in_len, uint32_t block_size, uint32_t element_size, uint32_t frame_step);
int         redux_lag_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                               uint32_t element_size, const uint32_t *lags /* host, nlags */, uint32_t nlags,
                               uint32_t frame_step, void *d_bits /* f64[nlags][block_count] */, void *stream);
const char *redux_lag_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t element_size);
const char *redux_lag_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size);

/* ---- order estimates -------------------------------------------------------------------------------------
 * The lag estimates above for higher-order lagged differences ("higher-order lagged differences" above): the adaptive cost A
 * of every block of the input behind the lag filter at order K, for a list of (lag, order) candidates in one call, so that
 * the order -- which pays on band-limited signals and costs bytes on random walks -- can be counted instead of guessed or
 * found by coding the input three times.  Nothing about the filter is new: bits[c][b] is what redux_block_cost_dev gives for
 * block b of what redux_lag_order_planes_dev writes for (element_size, block_size, lags[c], orders[c]) -- the fresh start of
 * every frame, terms before the frame zero, the fold, the short last frame and its trailing bytes included -- counted from
 * the untransformed bytes: no transformed copy and no workspace.  A candidate of order 1 gives redux_lag_cost_dev's row for
 * its lag.  Frame sampling (frame_step) and the compact rows are those of the lag estimates, and so is the row length,
 * redux_lag_cost_block_count.
 *
 * redux_lag_order_cost_dev             d_bits is f64[ncand][redux_lag_cost_block_count(...)] on the device.  lags, orders:
 *                                      ncand values each on the HOST, consumed before the call returns (they travel in the
 *                                      kernels' arguments); repeated candidates are legal, rows are independent.  The four
 *                                      waves of a workgroup take four consecutive candidates and move at the pace of the
 *                                      highest order among them: a list ordered by order first is the fastest (any order is
 *                                      right).
 *                                      Full frames go to k_lag_order_cost when block_size and d_in are multiples of 16,
 *                                      everything else (the short last frame included) to k_lag_order_cost_bytes, which is
 *                                      right for any alignment and block size but slow.  INVALID_INPUT where
 *                                      redux_lag_cost_dev returns it, for ncand == 0 or above REDUX_LAG_ORDER_COST_MAX, a
 *                                      null orders, or a pair redux_lag_order_check refuses; UNSUPPORTED as
 *                                      redux_block_cost_dev.  in_len == 0: one empty block per row.  Stream-ordered, no
 *                                      workspace, no host synchronisation.
 * redux_lag_order_cost_kernel_name     the kernels such a call with frame_step 1 runs on a 16-byte aligned d_in:
 *                                      "k_lag_order_cost<E>", "k_lag_order_cost_bytes<E>", or both joined by " + " when
 *                                      full frames are followed by a short one.  "" for a block_size or element size out of
 *                                      range.
 * redux_lag_order_cost_kernel_name_at  the same for this d_in, which contributes its alignment only. */
#define REDUX_LAG_ORDER_COST_MAX 256   /* candidates of one call */
int         redux_lag_order_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                                     uint32_t element_size, const uint32_t *lags /* host, ncand */,
                                     const uint32_t *orders /* host, ncand */, uint32_t ncand, uint32_t frame_step,
                                     void *d_bits /* f64[ncand][block_count] */, void *stream);
const char *redux_lag_order_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t element_size);
const char *redux_lag_order_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size);

/* ---- record estimates -----------------------------------------------------------------------------------
 * The adaptive model's cost of every block of the input behind the record layout, for a list of candidates (R, F): R a
 * record size redux_record_check accepts, F the byte delta (0 or 1).  bits[c][b] is what redux_block_cost_dev gives for
 * block b of what redux_record_planes_dev writes for candidate c, counted from the untransformed bytes: no transformed copy
 * and no workspace.  The fresh start of every frame of R * block_size bytes, the short last frame with its trailing bytes,
 * and in_len == 0 (one empty block per row) are part of the rule.
 *
 * Frame sampling.  Candidates have frames of different sizes, so the call takes sample_blocks Q in place of a frame step.
 * Q == 0 costs every frame.  For Q > 0, with nframes = max(1, ceil(in_len / (R * block_size))) and want = ceil(Q / R), the
 * step is T = 1 if nframes <= want and ceil(nframes / want) otherwise, and frames 0, T, 2T, ... are costed.  A candidate's
 * row is compact: the blocks of its selected frames in order, R per full frame, and what it has of a selected short last
 * frame.  Every row has the stride redux_block_count(in_len, block_size); entries past a row's own count are not written.
 *
 * redux_record_cost_frame_step       T for this candidate.  Host only, no GPU.  0 for a block_size outside 1 .. 2^30, a
 *                                    record size redux_record_check refuses, or a T above 2^32 - 1.
 * redux_record_cost_block_count      the blocks of the candidate's row.  Host only, no GPU.  0 for the same arguments.
 * redux_record_cost_dev              d_bits is f64[ncand][redux_block_count(in_len, block_size)] on the device.  records,
 *                                    deltas: ncand values each on the HOST, consumed before the call returns (they travel
 *                                    in the kernels' arguments); repeated candidates are legal, rows are independent, any
 *                                    order of the list is right.  Full frames go to k_record_cost when block_size and d_in
 *                                    are multiples of 16, everything else (the short last frame included) to
 *                                    k_record_cost_bytes, which is right for any alignment and block size but slow.
 *                                    INVALID_INPUT, with nothing written, for a block_size outside 1 .. 2^30, ncand == 0
 *                                    or above REDUX_RECORD_COST_MAX, a null list or d_bits, or a pair redux_record_check
 *                                    refuses; UNSUPPORTED as redux_block_cost_dev.  Stream-ordered, no workspace, no host
 *                                    synchronisation.
 * redux_record_cost_kernel_name      the kernels such a call with sample_blocks 0 runs on a 16-byte aligned d_in:
 *                                    "k_record_cost", "k_record_cost_bytes", or both joined by " + " when full frames are
 *                                    followed by a short one.  "" for a block_size or record size out of range.
 * redux_record_cost_kernel_name_at   the same for this d_in, which contributes its alignment only. */
#define REDUX_RECORD_COST_MAX 256   /* candidates of one call */
uint32_t    redux_record_cost_frame_step(uint64_t in_len, uint32_t block_size, uint32_t record_size, uint32_t sample_blocks);
uint64_t    redux_record_cost_block_count(uint64_t in_len, uint32_t block_size, uint32_t record_size, uint32_t sample_blocks);
int         redux_record_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                                  const uint32_t *records /* host, ncand */, const uint8_t *deltas /* host, ncand */,
                                  uint32_t ncand, uint32_t sample_blocks, void *d_bits /* f64[ncand][block_count] */,
                                  void *stream);
const char *redux_record_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t record_size);
const char *redux_record_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t record_size);

/* ---- mixed layouts --------------------------------------------------------------------------------------
 * One layout per UNIT of the input instead of one per input, for files that hold several element types (bf16 weights next to
 * fp32 state, int64 indices and text): the eight layouts of "layout estimates" above, chosen for every unit on its own.
 *
 * Unit         REDUX_MIXED_UNIT_BLOCKS (8) consecutive blocks, 8 * block_size bytes; only the last unit may be shorter;
 *              nunits = ceil(nblocks / 8).  The unit size is not a parameter.  8 is a multiple of every element size, so
 *              every unit boundary is a frame boundary of every layout.
 * Unit table   u8[nunits], entry k = 4 F + log2 E in 0 .. 7: the layout index of redux_layout_cost_dev.
 * Transform    the bytes of unit u of the result are the bytes of unit u of what redux_planes_dev (F = 0) or
 *              redux_delta_planes_dev (F = 1) writes for the WHOLE buffer under layout table[u]; layout 0 is a copy.  Frames
 *              start afresh and units are whole frames, so this is well defined, the short last unit with its short last
 *              frame and trailing bytes included.  The inverse undoes it unit by unit.
 * Choice       S[k][u] = the sum of bits[k][b] over the unit's blocks, added in f64 in ascending block order from 0.0;
 *              table[u] = the lowest selected k with the smallest S[k][u].  No hysteresis.
 *
 * On the device a table byte is taken & 7: no table content makes a kernel read or write outside [0, len).  A table in HOST
 * memory (the redux_*_blocks_mixed pair) with a byte above 7 is INVALID_INPUT before any launch.
 *
 * redux_mixed_unit_count            ceil(redux_block_count(in_len, block_size) / 8); 0 for block_size 0.
 * redux_mixed_choose_dev            d_bits f64[8][nblocks] (redux_layout_cost_dev's; only the rows of layouts_mask are read)
 *                                   -> d_table u8[ceil(nblocks / 8)] by the rule (k_mixed_choose).  d_sum_bits may be null:
 *                                   one u64 that receives the sum over the units of the chosen S, in units of
 *                                   2^-REDUX_MIXED_SUM_FRAC_BITS bit, each unit rounded to nearest.  INVALID_INPUT for
 *                                   layouts_mask == 0 or a bit above 7, null d_bits or d_table, nblocks == 0.
 * redux_mixed_layout_dev            the transform (inverse != 0: its inverse) of d_src[0 .. len) into d_dst, not in place.
 *                                   Full units go to k_mixed_planes when block_size and both pointers are multiples of 16,
 *                                   everything else (the short last unit included) to k_mixed_bytes, which is right for any
 *                                   alignment and block size but slow.  INVALID_INPUT for a block_size outside 1 .. 2^30
 *                                   or a null d_table.  Stream-ordered, no workspace.
 * redux_encode_mixed_dev            layouts_mask != 0: the costs of those layouts (redux_layout_cost_dev, rows in the
 *                                   workspace), the choice into d_table, the transform and the adaptive coder over it, all
 *                                   stream-ordered with no host synchronisation.  layouts_mask == 0: d_table is used as given.
 *                                   The rest as redux_encode_planes_dev.  INVALID_INPUT for a block_size outside 1 .. 2^30,
 *                                   mask bits above 7 or a null d_table; UNSUPPORTED where redux_block_cost_dev is.
 * redux_decode_mixed_dev            as redux_decode_planes_dev with the unit table in place of the element size: the blocks
 *                                   decode into the plane buffer of the workspace, their sizes are checked, and the inverse
 *                                   writes d_out[0 .. out_len) and nothing else.
 * redux_encode_blocks_mixed / redux_decode_blocks_mixed   the host-pointer pair on the chunk pipeline; `table` is
 *                                   u8[nunits] in host memory (written when layouts_mask != 0, read otherwise and by
 *                                   decode); block_crc may be null: the CRC-32 of every block of the original bytes.  The
 *                                   choice is per unit and chunks are whole units, so the result does not depend on the
 *                                   chunking.
 * redux_mixed_kernel_name           what redux_mixed_layout_dev runs on 16-byte aligned buffers: "k_mixed_planes<0>" (<1>:
 *                                   inverse), "k_mixed_bytes<0>", or both joined by " + " when full units are followed by a
 *                                   short one.  "" for a block_size out of range or len == 0.
 * redux_mixed_kernel_name_at        the same for these pointers, which contribute their alignment only. */
#define REDUX_MIXED_UNIT_BLOCKS 8
#define REDUX_MIXED_SUM_FRAC_BITS 16
uint64_t    redux_mixed_unit_count(uint64_t in_len, uint32_t block_size);
int         redux_mixed_choose_dev(const void *d_bits /* f64[8][nblocks] */, uint64_t nblocks, uint32_t layouts_mask,
                                   void *d_table /* u8[nunits] */, void *d_sum_bits /* u64, may be null */, void *stream);
int         redux_mixed_layout_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size,
                                   const void *d_table /* u8[nunits] */, int inverse, void *stream);
uint64_t    redux_encode_mixed_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size);
uint64_t    redux_decode_mixed_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size);
int         redux_encode_mixed_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                                   uint32_t layouts_mask, void *d_table /* u8[nunits] */, void *d_out, uint64_t out_cap,
                                   void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                                   uint64_t workspace_bytes, void *stream);
int         redux_decode_mixed_dev(const redux_params *p, const void *d_in, const void *d_in_offsets,
                                   const void *d_table /* u8[nunits] */, uint64_t out_len, uint32_t block_size, void *d_out,
                                   void *d_out_sizes, void *d_block_status, void *d_summary, void *d_workspace,
                                   uint64_t workspace_bytes, void *stream);
int         redux_encode_blocks_mixed(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                      uint32_t layouts_mask, uint8_t *table /* u8[nunits] */, uint8_t *out, uint64_t out_cap,
                                      uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc);
int         redux_decode_blocks_mixed(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets,
                                      const uint8_t *table /* u8[nunits] */, uint64_t out_len, uint32_t block_size, uint8_t *out,
                                      uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc);
const char *redux_mixed_kernel_name(uint64_t in_len, uint32_t block_size, int inverse);
const char *redux_mixed_kernel_name_at(const void *d_src, const void *d_dst, uint64_t in_len, uint32_t block_size, int inverse);

/* ---- range reads: decode only the blocks a byte range covers -----------------------------------------------------------
 * Blocks are coded independently, and every layout in front of the coder is local to a short run of blocks, the GRANULE of
 * g blocks: a frame of E blocks for the byte-plane layout, the delta filter, the XOR-against-base filter, stored and
 * constant blocks and plane-static coding (table b mod E); a unit of 8 blocks for the mixed layouts; a segment of
 * segment_blocks blocks for segment-static coding; one block (g = 1) where nothing sits in front of the coder.  Granule j of an
 * input of `total` bytes in blocks of B is blocks [j g, min((j + 1) g, nblocks)) and bytes [j g B, min((j + 1) g B, total)); only
 * the input's last granule can be short.
 *
 * Any run of whole granules -- its streams, its entries of the per-block tables (offsets rebased to 0, CRCs, stored and constant
 * flags), its entries of the per-unit table, its segments' tables, its bytes of the base -- is a valid smaller input of the
 * decode entry point of its layout, and so are several runs in ascending order, concatenated: the VIRTUAL INPUT.  The input's
 * short last granule, if a run holds it, comes last there as well, and a base that covered a prefix of the input covers a
 * prefix of the virtual input.  So reading R byte ranges is ONE decode call on the virtual input of the granules they cover,
 * whatever R, and each range is then a slice of the result.
 *
 * redux_range_plan is that geometry (host arithmetic, no device call).  The ranges (starts[i], lens[i]) may come in any order,
 * overlap and repeat.  Out: the union of the covered granules as disjoint ascending runs (run_first[r] the first granule,
 * run_count[r] granules; touching and overlapping intervals are merged, *nruns <= nranges); *virt_len the bytes of the virtual
 * input; virt_off[i] where range i begins in it.  A range without bytes covers no granule and gets virt_off 0 (starts[i] =
 * total_len included).  INVALID_INPUT: starts[i] > total_len, starts[i] + lens[i] > total_len (a sum that overflows 64 bits
 * included), block_size 0, granule_blocks 0. */
int redux_range_plan(uint64_t total_len, uint32_t block_size, uint64_t granule_blocks, const uint64_t *starts,
                     const uint64_t *lens, uint64_t nranges, uint64_t *run_first /* [nranges] */,
                     uint64_t *run_count /* [nranges] */, uint64_t *nruns, uint64_t *virt_off /* [nranges] */,
                     uint64_t *virt_len);

/* The device piece: a segmented byte copy driven by a table, dst[segs[i].dst ..][: len] = src[segs[i].src ..][: len] for
 * every i, both buffers at any byte alignment.  It gathers the covered streams of a compressed input kept in device memory
 * into one compact stream buffer (and the covered bytes of a base), and scatters the requested bytes out of the decoded
 * virtual input into the caller's tensor, without a host round trip.
 *
 * The segment table is HOST memory.  redux_segment_copy_dev checks it before any device call -- INVALID_INPUT for a segment
 * that leaves its buffer (src + len > src_bytes or dst + len > dst_bytes, overflow included), for destination segments that
 * overlap each other, and for buffers [d_src, d_src + src_bytes) and [d_dst, d_dst + dst_bytes) that overlap -- cuts the segments
 * into tiles of at most 64 KiB, uploads the tile table to the front of the workspace and launches k_segment_copy once,
 * stream-ordered (OUTPUT_TOO_SMALL for a workspace below redux_segment_copy_workspace_bytes).  No segments, or none with
 * bytes: OK, nothing is launched.  redux_segment_tiles is the cut: a tile never straddles a segment, the tiles of a segment
 * follow each other in order, and every tile but a segment's first starts at a 16-byte boundary of the destination (so only
 * a segment's ends take the kernel's byte path).  It returns the number of tiles and writes them when `tiles` is not NULL. */
typedef struct redux_segment {
    uint64_t src, dst, len; /* byte offsets into d_src / d_dst, and the bytes to copy */
} redux_segment;
uint64_t    redux_segment_copy_workspace_bytes(const redux_segment *segs, uint64_t nsegs);
uint64_t    redux_segment_tiles(const redux_segment *segs, uint64_t nsegs, redux_segment *tiles /* may be NULL */);
int         redux_segment_copy_dev(const void *d_src, uint64_t src_bytes, void *d_dst, uint64_t dst_bytes,
                                   const redux_segment *segs /* HOST memory */, uint64_t nsegs, void *d_workspace,
                                   uint64_t workspace_bytes, void *stream);
const char *redux_segment_copy_kernel_name(void);

/* Library / build identification: "redux_hip <version> gfx950". */
const char *redux_version(void);
/* sha256 (first 16 hex digits) of the kernel sources + this header the library was built from ("unknown" when the
 * build did not say): a profile records it, and a harness borrows a profiled figure only for the same sources. */
const char *redux_source_hash(void);

/* Which kernel redux_encode_slots_dev / redux_decode_blocks_dev launch for these arguments (the
 * same decision function the launch code uses; d_in / d_out only contribute their alignment).  A static
 * string; "" for invalid arguments.  A harness reports it next to its timings (bench.py's
 * roofline.kernel) instead of assuming the fast path was taken. */
const char *redux_encode_kernel_name(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size);
const char *redux_decode_kernel_name(const redux_params *p, const void *d_out, uint32_t block_size);
/* The encoder's choice also depends on the workspace the call is GIVEN: a launch the small-grid kernels would take runs the
 * full-grid kernels when workspace_bytes is below redux_encode_workspace_bytes' answer for its shape (no room for the pairs
 * area: every chunk of a multi-chunk host call).  redux_encode_kernel_name answers for a workspace of that size or more. */
const char *redux_encode_kernel_name_ws(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                                        uint64_t workspace_bytes);
/* The decoder also depends on the SIZE of the launch (blocks the lock-step decoder does not take -- above 64 KiB -- run one
 * per wave in launches of at most 1024 blocks, k_decode_wave, and on the cell decoder with u32 nodes, k_decode_cells<8>, in
 * larger ones; 11- and 12-bit symbols keep their bottom tree cells in LDS on small grids):
 * nblocks = blocks (or table entries) of the launch; 0 = a grid that fills the chip, which is what
 * redux_decode_kernel_name answers for. */
const char *redux_decode_kernel_name_n(const redux_params *p, const void *d_out, uint32_t block_size, uint64_t nblocks);
/* The decoder of a launch that is given a block table (redux_decode_blocks_v_dev; redux_decode_stored_dev, whose table has
 * one entry per block, so nentries = redux_block_count(out_len, block_size)): the cell decoder k_decode_cells<8> takes
 * blocks in order and has no table form, so blocks above 64 KiB in launches too big for k_decode_wave run k_decode<false,
 * true>.  "" for arguments the table form rejects (symbol_bits != 8 or code_bits > 32: UNSUPPORTED) and for nentries == 0. */
const char *redux_decode_kernel_name_table(const redux_params *p, uint32_t block_size, uint64_t nentries);
/* The same for redux_static_encode_blocks_dev / redux_static_decode_blocks_dev: the choice depends on the table total
 * (>= 2^17: quotient fix-up; <= 2^16: lookup-table decoder; between: lock-step decoder), on code_bits (32 or less) and on
 * whether the launch has at most one wave (64 blocks) per SIMD of HIP's current device.  Alignment is decided inside
 * the kernels.  "" for arguments the _dev call rejects, and for nblocks == 0 (the decode call launches nothing). */
const char *redux_static_encode_kernel_name(const redux_params *p, const uint32_t *cum, uint64_t in_len, uint32_t block_size);
const char *redux_static_decode_kernel_name(const redux_params *p, const uint32_t *cum, uint64_t nblocks);
/* The same for redux_plane_static_encode_dev / redux_plane_static_decode_dev, which run the k_*_segment_static* instances with
 * a single segment and report them under that name: the launch has element_size * ceil(ceil(nblocks / element_size) / 64)
 * waves. */
const char *redux_plane_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size,
                                                  uint32_t element_size);
const char *redux_plane_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks, uint32_t element_size);

/* The same for redux_segment_static_encode_dev / redux_segment_static_decode_dev (the k_*_segment_static* instances).  The
 * lookup decoder's 4 or 8 waves share one table and so one segment: it runs where k = segment_blocks / (64 element_size) is a
 * multiple of its wave count (8 not suiting, 4 is tried), and the lock-step decoder where neither suits. */
const char *redux_segment_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size,
                                                    uint32_t element_size, uint32_t segment_blocks);
const char *redux_segment_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks, uint32_t element_size,
                                                    uint32_t segment_blocks);

/* The same for redux_context_static_encode_dev / redux_context_static_decode_dev (the k_*_context_static instances): one
 * workgroup per CU holds the 128 KiB image, so the choice is the waves per workgroup, from the wave slots (64 blocks each) the
 * launch has per CU of HIP's current device: 4 up to 4 slots per CU, 8 up to 8 (the encoder's largest, also by code_bits 32
 * or less), 16 beyond (decoder only).  "" for arguments the _dev call rejects, and for nblocks == 0 (the decode call
 * launches nothing). */
const char *redux_context_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size);
const char *redux_context_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks);

/* Diagnostic, used by the parity tests only: *max_err = max over the integers x in [lo, hi] of
 * |v_rcp_f64(x) * x - 1| evaluated on the device.  The decoder's code-value division
 * (codec.rs:131) multiplies by the raw hardware reciprocal of `range` (an integer in [1, 2^32])
 * and relies on this error staying below 2^-24 over that whole range. */
int redux_debug_rcp_check(uint64_t lo, uint64_t hi, double *max_err);

/* Diagnostic, used by the parity tests only: byte offset and length, inside the encode workspace
 * of (p, in_len, block_size), of the encoder's per-CU role book (see redux_encode.hpp).  Every
 * encode workgroup returns its booking when it ends, so the region reads all-zero after a
 * completed redux_encode_slots_dev / redux_encode_blocks_dev. */
int redux_debug_role_book(const redux_params *p, uint64_t in_len, uint32_t block_size, uint64_t *offset,
                          uint64_t *bytes);

/* Diagnostic, used by the tests only: the tile height of the encoder's row gather (k_compact_rows, which places the streams
 * a pair or small-grid kernel left in row-major group areas).  The launch code takes tiles of 256 rows where a slot is at least
 * four of them long (4 KiB) and tiles of 64 rows below; rows = 64 or 256 makes every later call of this process use that
 * instance whatever the slot size, rows = 0 gives the choice back.  The dense output does not depend on it.  INVALID_INPUT
 * for any other value. */
int redux_debug_compact_tile_rows(uint32_t rows);

#ifdef __cplusplus
}
#endif
#endif
