//! MI355X block coder behind `redux::compress` / `redux::decompress`.
//!
//! Drop this file into the reference crate as `src/hip.rs` and declare it from `src/lib.rs` with
//! `pub mod hip;`.  It binds the C ABI of `include/redux_hip.h` (libredux_hip.so) and contains no
//! coding logic: only argument marshalling and the mapping of status codes onto `redux::Error`
//! (src/lib.rs:57-64).  Rust 2015 edition, like the crate (`try!`, bare trait objects).
//!
//! Acceleration is selected BY API: `Box<Model>` is an open trait object the GPU cannot call back
//! into, so these functions take `&Parameters` and always code with the semantics of
//! `AdaptiveTreeModel::new(params.clone())` (src/model/adaptive_tree.rs:36).  The existing
//! `compress` / `decompress` / `Codec` / `Model` surface is untouched.
//!
//! `tests/test_rust_shim_cpu.py` in the redux_amd repository parses the `extern "C"` block below and
//! checks every declaration against `include/redux_hip.h` (name, arity, pointer-vs-integer and
//! integer width of each argument and of the return type).
use std::io;
use std::os::raw::{c_char, c_int, c_void};
use std::ptr;

use super::model::Parameters;
use super::{Error, Result};

/// `redux_params` of include/redux_hip.h: the three arguments of `Parameters::new`
/// (src/model/mod.rs:63); the library derives the other eight fields itself.
#[repr(C)]
pub struct ReduxParams {
    symbol_bits: u32,
    freq_bits: u32,
    code_bits: u32,
}

extern "C" {
    fn redux_params_check(symbol_bits: u32, freq_bits: u32, code_bits: u32) -> c_int;
    fn redux_device_supports(p: *const ReduxParams) -> c_int;
    fn redux_block_count(in_len: u64, block_size: u32) -> u64;
    fn redux_encode_bound(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    fn redux_encode_blocks(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32,
                           out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                           block_status: *mut i32) -> c_int;
    fn redux_decode_blocks(p: *const ReduxParams, input: *const u8, in_offsets: *const u64,
                           nblocks: u64, block_size: u32, out: *mut u8, out_cap: u64,
                           out_sizes: *mut u32, block_status: *mut i32) -> c_int;
    fn redux_block_count_v(in_len: *const u64, ninputs: u64, block_size: u32) -> u64;
    fn redux_encode_slot_bytes(p: *const ReduxParams, block_size: u32) -> u64;
    fn redux_encode_blocks_v(p: *const ReduxParams, input: *const u8, in_off: *const u64, in_len: *const u64,
                             ninputs: u64, block_size: u32, out: *mut u8, out_cap: u64,
                             out_offsets: *mut u64, block_status: *mut i32) -> c_int;
    fn redux_decode_blocks_v(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out: *mut u8,
                             out_off: *const u64, out_len: *const u64, ninputs: u64, block_size: u32,
                             out_sizes: *mut u32, block_status: *mut i32) -> c_int;
    fn redux_compress(p: *const ReduxParams, input: *const u8, in_len: u64, out: *mut u8,
                      out_cap: u64, bytes_in: *mut u64, bytes_out: *mut u64) -> c_int;
    fn redux_decompress(p: *const ReduxParams, input: *const u8, in_len: u64, out: *mut u8,
                        out_cap: u64, bytes_in: *mut u64, bytes_out: *mut u64) -> c_int;
    fn redux_encode_blocks_planes(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                  out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32) -> c_int;
    fn redux_decode_blocks_planes(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                  block_size: u32, element_size: u32, out: *mut u8, out_sizes: *mut u32,
                                  block_status: *mut i32) -> c_int;
    // delta filter for integer series, in front of the byte-plane layout (block_crc may be null)
    fn redux_encode_blocks_delta(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                 out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                                 block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_delta(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                 block_size: u32, element_size: u32, out: *mut u8, out_sizes: *mut u32,
                                 block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // zigzag-folded delta filter for signed series: the delta calls' shape
    fn redux_encode_blocks_zigzag(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                  out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                                  block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_zigzag(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                  block_size: u32, element_size: u32, out: *mut u8, out_sizes: *mut u32,
                                  block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // lagged delta filter for interleaved channels: the zigzag calls' shape with the lag behind the element size
    fn redux_encode_blocks_lag(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                               lag: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                               block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_lag(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                               block_size: u32, element_size: u32, lag: u32, out: *mut u8, out_sizes: *mut u32,
                               block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // higher-order lagged differences: the lag calls' shape with the order behind the lag
    fn redux_encode_blocks_lag_order(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                     lag: u32, order: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                     block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_lag_order(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                     block_size: u32, element_size: u32, lag: u32, order: u32, out: *mut u8,
                                     out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // record layout for fixed-width structs: the lag calls' shape with (record size, delta flag) in place of (element size, lag)
    fn redux_encode_blocks_record(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, record_size: u32,
                                  delta: c_int, out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                                  block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_record(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                  block_size: u32, record_size: u32, delta: c_int, out: *mut u8, out_sizes: *mut u32,
                                  block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // snapshot-stride filter for time series of fields: the lag calls' shape with the stride, a u64, where the lag is.  The pair
    // stages the whole buffer on one device (include/redux_hip.h, "snapshot-stride filter")
    fn redux_stride_check(element_size: u32, stride: u64) -> c_int;
    fn redux_encode_blocks_stride(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                  stride: u64, out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                                  block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_stride(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                  block_size: u32, element_size: u32, stride: u64, out: *mut u8, out_sizes: *mut u32,
                                  block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // XOR-against-base filter for series of snapshots, in front of the byte-plane layout (base null only with base_len 0;
    // block_crc may be null)
    fn redux_encode_blocks_base(p: *const ReduxParams, input: *const u8, in_len: u64, base: *const u8, base_len: u64,
                                block_size: u32, element_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_base(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, base: *const u8,
                                base_len: u64, out_len: u64, block_size: u32, element_size: u32, out: *mut u8,
                                out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // folded difference against a base: the base filter's other operation, the arguments of the pair above
    fn redux_encode_blocks_base_sub(p: *const ReduxParams, input: *const u8, in_len: u64, base: *const u8, base_len: u64,
                                    block_size: u32, element_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                    block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_base_sub(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, base: *const u8,
                                    base_len: u64, out_len: u64, block_size: u32, element_size: u32, out: *mut u8,
                                    out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // constant blocks: a block of equal bytes travels as one byte (base null only with base_len 0: no base; block_crc may
    // be null)
    fn redux_encode_blocks_const(p: *const ReduxParams, input: *const u8, in_len: u64, base: *const u8, base_len: u64,
                                 block_size: u32, element_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                 const_flags: *mut u8, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_const(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, const_flags: *const u8,
                                 base: *const u8, base_len: u64, out_len: u64, block_size: u32, element_size: u32,
                                 out: *mut u8, out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // lag estimates: the adaptive cost of every block behind the lagged delta filter for a list of lags (device pointers;
    // declared for callers that hold device buffers, not used by the host-slice functions below)
    #[allow(dead_code)]
    fn redux_lag_cost_block_count(in_len: u64, block_size: u32, element_size: u32, frame_step: u32) -> u64;
    #[allow(dead_code)]
    fn redux_lag_cost_dev(p: *const ReduxParams, d_in: *const c_void, in_len: u64, block_size: u32, element_size: u32,
                          lags: *const u32, nlags: u32, frame_step: u32, d_bits: *mut c_void, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_lag_cost_kernel_name(in_len: u64, block_size: u32, element_size: u32) -> *const c_char;
    #[allow(dead_code)]
    fn redux_lag_cost_kernel_name_at(d_in: *const c_void, in_len: u64, block_size: u32, element_size: u32) -> *const c_char;
    // order estimates: the same for a list of (lag, order) candidates of higher-order lagged differences
    #[allow(dead_code)]
    fn redux_lag_order_cost_dev(p: *const ReduxParams, d_in: *const c_void, in_len: u64, block_size: u32, element_size: u32,
                                lags: *const u32, orders: *const u32, ncand: u32, frame_step: u32, d_bits: *mut c_void,
                                stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_lag_order_cost_kernel_name(in_len: u64, block_size: u32, element_size: u32) -> *const c_char;
    #[allow(dead_code)]
    fn redux_lag_order_cost_kernel_name_at(d_in: *const c_void, in_len: u64, block_size: u32, element_size: u32) -> *const c_char;
    // record estimates: the cost behind the record layout for a list of (record size, delta) candidates, with its sampling
    #[allow(dead_code)]
    fn redux_record_cost_frame_step(in_len: u64, block_size: u32, record_size: u32, sample_blocks: u32) -> u32;
    #[allow(dead_code)]
    fn redux_record_cost_block_count(in_len: u64, block_size: u32, record_size: u32, sample_blocks: u32) -> u64;
    #[allow(dead_code)]
    fn redux_record_cost_dev(p: *const ReduxParams, d_in: *const c_void, in_len: u64, block_size: u32, records: *const u32,
                             deltas: *const u8, ncand: u32, sample_blocks: u32, d_bits: *mut c_void, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_record_cost_kernel_name(in_len: u64, block_size: u32, record_size: u32) -> *const c_char;
    #[allow(dead_code)]
    fn redux_record_cost_kernel_name_at(d_in: *const c_void, in_len: u64, block_size: u32, record_size: u32) -> *const c_char;
    fn redux_static_table_check(p: *const ReduxParams, cum: *const u32) -> c_int;
    fn redux_static_encode_bound(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    fn redux_static_table_from_counts(p: *const ReduxParams, counts: *const u64, total: u32, cum: *mut u32) -> c_int;
    fn redux_static_table(p: *const ReduxParams, input: *const u8, in_len: u64, total: u32, cum: *mut u32) -> c_int;
    fn redux_static_encode_blocks(p: *const ReduxParams, cum: *const u32, input: *const u8, in_len: u64, block_size: u32,
                                  out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32) -> c_int;
    fn redux_static_decode_blocks(p: *const ReduxParams, cum: *const u32, input: *const u8, in_offsets: *const u64,
                                  nblocks: u64, block_size: u32, out: *mut u8, out_cap: u64, out_sizes: *mut u32,
                                  block_status: *mut i32) -> c_int;
    fn redux_crc32_combine(crc1: u32, crc2: u32, len2: u64) -> u32;
    fn redux_crc32_blocks(input: *const u8, in_len: u64, block_size: u32, crc: *mut u32) -> c_int;
    fn redux_encode_blocks_crc(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, out: *mut u8,
                               out_cap: u64, out_offsets: *mut u64, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_crc(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, nblocks: u64,
                               block_size: u32, out: *mut u8, out_cap: u64, out_sizes: *mut u32, block_status: *mut i32,
                               block_crc: *mut u32) -> c_int;
    fn redux_encode_blocks_planes_crc(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32,
                                      element_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                      block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_planes_crc(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, out_len: u64,
                                      block_size: u32, element_size: u32, out: *mut u8, out_sizes: *mut u32,
                                      block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_static_encode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_len: u64,
                                      block_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                      block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_static_decode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_offsets: *const u64,
                                      nblocks: u64, block_size: u32, out: *mut u8, out_cap: u64, out_sizes: *mut u32,
                                      block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // plane-static coding: one static table per byte plane (cum: u32[element_size][258])
    fn redux_plane_static_table_check(p: *const ReduxParams, cum: *const u32, element_size: u32) -> c_int;
    fn redux_plane_static_total(cum: *const u32, element_size: u32) -> u32;
    fn redux_plane_static_tables_from_counts(p: *const ReduxParams, counts: *const u64, element_size: u32, total: u32,
                                             cum: *mut u32) -> c_int;
    fn redux_plane_static_tables(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                 total: u32, cum: *mut u32) -> c_int;
    fn redux_plane_static_encode_bound(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    fn redux_plane_static_encode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_len: u64,
                                            block_size: u32, element_size: u32, out: *mut u8, out_cap: u64,
                                            out_offsets: *mut u64, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_plane_static_decode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_offsets: *const u64,
                                            out_len: u64, block_size: u32, element_size: u32, out: *mut u8,
                                            out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    // segment-static coding: static tables per range of segment_blocks blocks (cum: u32[nseg * element_size][258])
    fn redux_segment_static_table_count(nblocks: u64, element_size: u32, segment_blocks: u32) -> u64;
    #[allow(dead_code)]
    fn redux_segment_static_table_check(p: *const ReduxParams, cum: *const u32, ntables: u64, nblocks: u64, element_size: u32,
                                        segment_blocks: u32) -> c_int;
    #[allow(dead_code)]
    fn redux_segment_static_total(cum: *const u32, ntables: u64) -> u32;
    #[allow(dead_code)]
    fn redux_segment_static_tables_from_counts(p: *const ReduxParams, counts: *const u64, nblocks: u64, element_size: u32,
                                               segment_blocks: u32, total: u32, cum: *mut u32) -> c_int;
    fn redux_segment_static_encode_bound(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    fn redux_segment_static_encode_blocks_crc(p: *const ReduxParams, total: u32, input: *const u8, in_len: u64, block_size: u32,
                                              element_size: u32, segment_blocks: u32, cum: *mut u32, out: *mut u8, out_cap: u64,
                                              out_offsets: *mut u64, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_segment_static_decode_blocks_crc(p: *const ReduxParams, cum: *const u32, ntables: u64, input: *const u8,
                                              in_offsets: *const u64, out_len: u64, block_size: u32, element_size: u32,
                                              segment_blocks: u32, out: *mut u8, out_sizes: *mut u32, block_status: *mut i32,
                                              block_crc: *mut u32) -> c_int;
    // context-static coding: a static table per preceding byte (cum: u32[256][258])
    fn redux_context_static_table_check(p: *const ReduxParams, cum: *const u32) -> c_int;
    fn redux_context_static_total(cum: *const u32) -> u32;
    fn redux_context_static_tables_from_counts(p: *const ReduxParams, counts: *const u64, total: u32, cum: *mut u32) -> c_int;
    fn redux_context_static_tables(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, total: u32,
                                   cum: *mut u32) -> c_int;
    fn redux_context_static_encode_bound(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    fn redux_context_static_encode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_len: u64,
                                              block_size: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64,
                                              block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_context_static_decode_blocks_crc(p: *const ReduxParams, cum: *const u32, input: *const u8, in_offsets: *const u64,
                                              nblocks: u64, block_size: u32, out: *mut u8, out_cap: u64, out_sizes: *mut u32,
                                              block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_encode_blocks_stored(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, element_size: u32,
                                  store_ratio: u32, out: *mut u8, out_cap: u64, out_offsets: *mut u64, stored: *mut u8,
                                  block_status: *mut i32, block_crc: *mut u32) -> c_int;
    fn redux_decode_blocks_stored(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, stored: *const u8,
                                  out_len: u64, block_size: u32, element_size: u32, out: *mut u8, out_cap: u64,
                                  out_sizes: *mut u32, block_status: *mut i32, block_crc: *mut u32) -> c_int;
    #[allow(dead_code)] // declared for harnesses that print the kernel next to a timing; no wrapper here
    fn redux_encode_kernel_name_ws(p: *const ReduxParams, d_in: *const c_void, in_len: u64, block_size: u32,
                                   workspace_bytes: u64) -> *const c_char;
    #[allow(dead_code)] // the same for the decoder a stored launch runs (the table form)
    fn redux_decode_kernel_name_table(p: *const ReduxParams, block_size: u32, nentries: u64) -> *const c_char;
    #[allow(dead_code)] // the same for the context-static coders: which of their seven instances a launch runs
    fn redux_context_static_encode_kernel_name(p: *const ReduxParams, total: u32, in_len: u64, block_size: u32) -> *const c_char;
    #[allow(dead_code)]
    fn redux_context_static_decode_kernel_name(p: *const ReduxParams, total: u32, nblocks: u64) -> *const c_char;
    // mixed layouts: a layout per unit of 8 blocks (table: u8[redux_mixed_unit_count]); declared for callers that keep
    // their data on the device or write their own container, no wrapper here
    #[allow(dead_code)]
    fn redux_mixed_unit_count(in_len: u64, block_size: u32) -> u64;
    #[allow(dead_code)]
    fn redux_mixed_choose_dev(d_bits: *const c_void, nblocks: u64, layouts_mask: u32, d_table: *mut c_void,
                              d_sum_bits: *mut c_void, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_mixed_layout_dev(d_src: *const c_void, d_dst: *mut c_void, len: u64, block_size: u32, d_table: *const c_void,
                              inverse: c_int, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_encode_mixed_workspace_bytes(p: *const ReduxParams, in_len: u64, block_size: u32) -> u64;
    #[allow(dead_code)]
    fn redux_decode_mixed_workspace_bytes(p: *const ReduxParams, out_len: u64, block_size: u32) -> u64;
    #[allow(dead_code)]
    fn redux_encode_mixed_dev(p: *const ReduxParams, d_in: *const c_void, in_len: u64, block_size: u32, layouts_mask: u32,
                              d_table: *mut c_void, d_out: *mut c_void, out_cap: u64, d_out_offsets: *mut c_void,
                              d_block_status: *mut c_void, d_summary: *mut c_void, d_workspace: *mut c_void,
                              workspace_bytes: u64, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_decode_mixed_dev(p: *const ReduxParams, d_in: *const c_void, d_in_offsets: *const c_void, d_table: *const c_void,
                              out_len: u64, block_size: u32, d_out: *mut c_void, d_out_sizes: *mut c_void,
                              d_block_status: *mut c_void, d_summary: *mut c_void, d_workspace: *mut c_void,
                              workspace_bytes: u64, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn redux_encode_blocks_mixed(p: *const ReduxParams, input: *const u8, in_len: u64, block_size: u32, layouts_mask: u32,
                                 table: *mut u8, out: *mut u8, out_cap: u64, out_offsets: *mut u64, block_status: *mut i32,
                                 block_crc: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn redux_decode_blocks_mixed(p: *const ReduxParams, input: *const u8, in_offsets: *const u64, table: *const u8,
                                 out_len: u64, block_size: u32, out: *mut u8, out_sizes: *mut u32, block_status: *mut i32,
                                 block_crc: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn redux_mixed_kernel_name(in_len: u64, block_size: u32, inverse: c_int) -> *const c_char;
    #[allow(dead_code)]
    fn redux_mixed_kernel_name_at(d_src: *const c_void, d_dst: *const c_void, in_len: u64, block_size: u32,
                                  inverse: c_int) -> *const c_char;
    // range reads: the plan of the granules a set of byte ranges covers (host arithmetic).  The segmented copy's calls
    // (redux_segment_tiles, redux_segment_copy_workspace_bytes, redux_segment_copy_dev) take tables of the struct
    // redux_segment and are for callers that keep streams in device memory: not bound here.
    #[allow(dead_code)]
    fn redux_range_plan(total_len: u64, block_size: u32, granule_blocks: u64, starts: *const u64, lens: *const u64,
                        nranges: u64, run_first: *mut u64, run_count: *mut u64, nruns: *mut u64, virt_off: *mut u64,
                        virt_len: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn redux_segment_copy_kernel_name() -> *const c_char;
    fn redux_host_release() -> c_int;
    fn redux_host_set_devices(device_ids: *const i32, n: u32) -> c_int;
}

/// Status codes of include/redux_hip.h -> `redux::Error` (src/lib.rs:57-64).
fn status(st: c_int) -> Result<()> {
    match st {
        0 => Ok(()),
        1 => Err(Error::Eof),
        2 => Err(Error::InvalidInput),
        4 => Err(Error::IoError(io::Error::new(io::ErrorKind::Other, "redux_hip: output too small"))),
        5 => Err(Error::IoError(io::Error::new(io::ErrorKind::Other, "redux_hip: parameters unsupported on the device"))),
        _ => Err(Error::IoError(io::Error::new(io::ErrorKind::Other, "redux_hip: HIP runtime error"))),
    }
}

fn c_params(p: &Parameters) -> ReduxParams {
    ReduxParams { symbol_bits: p.symbol_bits as u32, freq_bits: p.freq_bits as u32, code_bits: p.code_bits as u32 }
}

/// `true` when the device implements these parameters (`symbol_bits <= 16`); a caller may route
/// everything else to the pure-Rust `redux::compress`.  The library itself has no CPU fallback.
pub fn supports(p: &Parameters) -> bool {
    let cp = c_params(p);
    unsafe {
        redux_params_check(cp.symbol_bits, cp.freq_bits, cp.code_bits) == 0 && redux_device_supports(&cp) == 0
    }
}

/// The library keeps one lazily built, mutex-guarded context per GPU for these calls (chunk slots in HBM, pinned
/// staging, streams), grown on demand and reused: calls from several threads are safe and run one after the other.
/// `release` frees it (it is rebuilt by the next call); a long-lived process that is done coding may call it.
pub fn release() {
    unsafe {
        redux_host_release();
    }
}

/// Several GPUs behind `compress_blocks` / `decompress_blocks`: every later call deals its chunks round-robin over one
/// context per entry of `device_ids` (each fed over its own PCIe link; the devices exchange nothing).  An empty slice
/// goes back to the default, HIP's current device.
pub fn set_devices(device_ids: &[i32]) -> Result<()> {
    unsafe { status(redux_host_set_devices(if device_ids.is_empty() { ptr::null() } else { device_ids.as_ptr() }, device_ids.len() as u32)) }
}

/// One `redux::compress` per block of `block_size` bytes, all blocks coded in parallel on the GPU.
/// Returns the dense streams and `nblocks + 1` offsets; block `b` is
/// `out[offsets[b] as usize..offsets[b + 1] as usize]` and is byte-identical to
/// `redux::compress(&mut &data[b * block_size..][..len_b], .., AdaptiveTreeModel::new(p.clone()))`.
pub fn compress_blocks(data: &[u8], block_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks(&cp, data.as_ptr(), data.len() as u64, block_size,
                                        out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks`: block `b` of the result is `out[b * block_size..][..sizes[b]]`.
pub fn decompress_blocks(streams: &[u8], offsets: &[u64], block_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u32>)> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    let nb = offsets.len() - 1;
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let mut out = vec![0u8; nb * block_size as usize];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks(&cp, streams.as_ptr(), offsets.as_ptr(), nb as u64, block_size,
                                        out.as_mut_ptr(), out.len() as u64, sizes.as_mut_ptr(), ptr::null_mut())));
        Ok((out, sizes))
    }
}

/// `compress_blocks` of typed data in the byte-plane layout (include/redux_hip.h): `element_size` 2, 4 or 8 (bf16 / fp16,
/// fp32 / i32, f64 / i64; 1 = no layout, the same streams as `compress_blocks`).  Frames of `element_size * block_size`
/// bytes are transformed so that each block holds one byte plane, then coded exactly as `compress_blocks` codes them.
pub fn compress_blocks_planes(data: &[u8], block_size: u32, element_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_planes(&cp, data.as_ptr(), data.len() as u64, block_size, element_size,
                                               out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_planes`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_planes(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, element_size: u32,
                                p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_planes(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, element_size,
                                               out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks` of an integer series behind the delta filter (include/redux_hip.h, "delta filter"): `element_size` 1, 2,
/// 4 or 8; the differences of neighbouring little-endian unsigned elements are coded, frame by frame of the byte-plane
/// layout.  Opt-in: floating-point data and text get larger with it.
pub fn compress_blocks_delta(data: &[u8], block_size: u32, element_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_delta(&cp, data.as_ptr(), data.len() as u64, block_size, element_size,
                                              out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_delta`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_delta(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, element_size: u32,
                               p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_delta(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, element_size,
                                              out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks_delta` with every difference zigzag-folded (include/redux_hip.h, "zigzag-folded delta filter"): for
/// series that move both ways, whose small negative differences would otherwise fill the upper byte planes with 0xFF.
pub fn compress_blocks_zigzag(data: &[u8], block_size: u32, element_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_zigzag(&cp, data.as_ptr(), data.len() as u64, block_size, element_size,
                                               out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_zigzag`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_zigzag(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, element_size: u32,
                                p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_zigzag(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, element_size,
                                               out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks_zigzag` with the predecessor `lag` elements back, 1 to 256 (include/redux_hip.h, "lagged delta
/// filter"): for `lag` interleaved channels or records of `lag` columns.  Opt-in: a wrong lag costs bytes.
pub fn compress_blocks_lag(data: &[u8], block_size: u32, element_size: u32, lag: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_lag(&cp, data.as_ptr(), data.len() as u64, block_size, element_size, lag,
                                            out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_lag` with the same `lag`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_lag(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, element_size: u32, lag: u32,
                             p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_lag(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, element_size, lag,
                                            out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks_lag` with the lag-`lag` difference applied `order` times, 1 to 3 (include/redux_hip.h, "higher-order
/// lagged differences"): for sampled signals that are locally polynomial.  Order 1 gives `compress_blocks_lag`'s streams.
/// Opt-in: on random walks a higher order costs bytes.
pub fn compress_blocks_lag_order(data: &[u8], block_size: u32, element_size: u32, lag: u32, order: u32,
                                 p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_lag_order(&cp, data.as_ptr(), data.len() as u64, block_size, element_size, lag, order,
                                                  out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(),
                                                  ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_lag_order` with the same `lag` and `order`: `len` is the original byte count; returns the
/// original bytes.
pub fn decompress_blocks_lag_order(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, element_size: u32, lag: u32,
                                   order: u32, p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_lag_order(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, element_size, lag,
                                                  order, out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(),
                                                  ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks` behind the record layout for fixed-width structs (include/redux_hip.h, "record layout"): every block
/// holds one byte column of `block_size` records of `record_size` bytes, 2 to 256; `delta`: the byte delta against the
/// record before.  Opt-in.
pub fn compress_blocks_record(data: &[u8], block_size: u32, record_size: u32, delta: bool,
                              p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_record(&cp, data.as_ptr(), data.len() as u64, block_size, record_size, delta as c_int,
                                               out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(),
                                               ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_record` with the same `record_size` and `delta`: `len` is the original byte count; returns
/// the original bytes.
pub fn decompress_blocks_record(streams: &[u8], offsets: &[u64], len: u64, block_size: u32, record_size: u32, delta: bool,
                                p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_record(&cp, streams.as_ptr(), offsets.as_ptr(), len, block_size, record_size,
                                               delta as c_int, out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(),
                                               ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks` of a snapshot behind the XOR-against-base filter (include/redux_hip.h, "XOR-against-base filter"):
/// `base` is an earlier snapshot of the same data, of any length; the bytewise XOR against it is coded in the byte-plane
/// layout of `element_size` 1, 2, 4 or 8.  Opt-in, and the decoder needs the same base.
pub fn compress_blocks_base(data: &[u8], base: &[u8], block_size: u32, element_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_base(&cp, data.as_ptr(), data.len() as u64, base.as_ptr(), base.len() as u64, block_size,
                                             element_size, out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut(),
                                             ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_base`, with the same `base`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_base(streams: &[u8], offsets: &[u64], base: &[u8], len: u64, block_size: u32, element_size: u32,
                              p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_base(&cp, streams.as_ptr(), offsets.as_ptr(), base.as_ptr(), base.len() as u64, len,
                                             block_size, element_size, out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(),
                                             ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks` of a snapshot behind the folded difference against a base (include/redux_hip.h, "folded difference
/// against a base"): `compress_blocks_base` with the zigzag-folded difference of the little-endian elements in place of the
/// XOR.  Opt-in, and the decoder needs the same base.
pub fn compress_blocks_base_sub(data: &[u8], base: &[u8], block_size: u32, element_size: u32, p: &Parameters)
                                -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_base_sub(&cp, data.as_ptr(), data.len() as u64, base.as_ptr(), base.len() as u64,
                                                 block_size, element_size, out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(),
                                                 ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_base_sub`, with the same `base`: `len` is the original byte count; returns the original bytes.
pub fn decompress_blocks_base_sub(streams: &[u8], offsets: &[u64], base: &[u8], len: u64, block_size: u32, element_size: u32,
                                  p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_base_sub(&cp, streams.as_ptr(), offsets.as_ptr(), base.as_ptr(), base.len() as u64, len,
                                                 block_size, element_size, out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(),
                                                 ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// `compress_blocks` with constant blocks skipped (include/redux_hip.h, "constant blocks"): a block of the coder's input --
/// the bytes, their byte-plane layout of `element_size` 1, 2, 4 or 8, or the layout of data ^ base when `base` is not empty
/// -- whose bytes are all equal has that one byte as its payload.  Returns (streams, offsets, flags); the decoder needs the
/// flags and the same base.  Opt-in.
pub fn compress_blocks_const(data: &[u8], base: &[u8], block_size: u32, element_size: u32, p: &Parameters)
                             -> Result<(Vec<u8>, Vec<u64>, Vec<u8>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        let mut flags = vec![0u8; nb];
        try!(status(redux_encode_blocks_const(&cp, data.as_ptr(), data.len() as u64, base.as_ptr(), base.len() as u64, block_size,
                                              element_size, out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), flags.as_mut_ptr(),
                                              ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs, flags))
    }
}

/// Inverse of `compress_blocks_const`, with its flags and the same `base`: `len` is the original byte count; returns the
/// original bytes.
pub fn decompress_blocks_const(streams: &[u8], offsets: &[u64], flags: &[u8], base: &[u8], len: u64, block_size: u32,
                               element_size: u32, p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count(len, block_size) as usize;
        if nb + 1 != offsets.len() || nb != flags.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(len as usize, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_const(&cp, streams.as_ptr(), offsets.as_ptr(), flags.as_ptr(), base.as_ptr(),
                                              base.len() as u64, len, block_size, element_size, out.as_mut_ptr(),
                                              sizes.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// The table total used when none is given: `min(2^16, freq_max)`, which keeps the table on the lookup decoder.
pub fn default_static_total(p: &Parameters) -> u32 {
    std::cmp::min(1u64 << 16, (1u64 << p.freq_bits) - 1) as u32
}

/// Semi-static coding (include/redux_hip.h): the static table `cum[0..=257]` of 256 byte counts by the documented rule,
/// computed on the host (no GPU).
pub fn static_table_from_counts(counts: &[u64; 256], total: u32, p: &Parameters) -> Result<Vec<u32>> {
    let cp = c_params(p);
    let mut cum = vec![0u32; 258];
    unsafe {
        try!(status(redux_static_table_from_counts(&cp, counts.as_ptr(), total, cum.as_mut_ptr())));
    }
    Ok(cum)
}

/// The static table of `data`: its bytes are counted on the current GPU, then the rule is applied.
pub fn static_table(data: &[u8], total: u32, p: &Parameters) -> Result<Vec<u32>> {
    let cp = c_params(p);
    let mut cum = vec![0u32; 258];
    unsafe {
        try!(status(redux_static_table(&cp, data.as_ptr(), data.len() as u64, total, cum.as_mut_ptr())));
    }
    Ok(cum)
}

/// `compress_blocks` under the fixed table `cum` (258 entries, e.g. from `static_table`) instead of the adaptive model.
pub fn compress_blocks_static(data: &[u8], block_size: u32, cum: &[u32], p: &Parameters) -> Result<(Vec<u8>, Vec<u64>)> {
    if block_size == 0 || cum.len() != 258 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        try!(status(redux_static_table_check(&cp, cum.as_ptr())));
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let cap = redux_static_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_static_encode_blocks(&cp, cum.as_ptr(), data.as_ptr(), data.len() as u64, block_size,
                                               out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs))
    }
}

/// Inverse of `compress_blocks_static`: block `b` of the result is `out[b * block_size..][..sizes[b]]`.
pub fn decompress_blocks_static(streams: &[u8], offsets: &[u64], block_size: u32, cum: &[u32],
                                p: &Parameters) -> Result<(Vec<u8>, Vec<u32>)> {
    if block_size == 0 || cum.len() != 258 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    let nb = offsets.len() - 1;
    unsafe {
        try!(status(redux_static_table_check(&cp, cum.as_ptr())));
        let mut out = vec![0u8; nb * block_size as usize];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_static_decode_blocks(&cp, cum.as_ptr(), streams.as_ptr(), offsets.as_ptr(), nb as u64, block_size,
                                               out.as_mut_ptr(), out.len() as u64, sizes.as_mut_ptr(), ptr::null_mut())));
        Ok((out, sizes))
    }
}

/// Segment-static coding (include/redux_hip.h): static tables per range of `segment_blocks` = 64 * `element_size` * k blocks
/// of the byte-plane layout, built from each range as it is coded.  Returns the dense streams, `nblocks + 1` offsets and the
/// tables (`nseg * element_size * 258` entries).  `total` 0: min(2^16, freq_max).
pub fn compress_blocks_segment_static(data: &[u8], block_size: u32, element_size: u32, segment_blocks: u32, total: u32,
                                      p: &Parameters) -> Result<(Vec<u8>, Vec<u64>, Vec<u32>)> {
    if block_size == 0 {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    let fmax = (1u64 << cp.freq_bits) - 1;
    let total = if total == 0 { if fmax < 65536 { fmax as u32 } else { 65536 } } else { total };
    unsafe {
        let nb = redux_block_count(data.len() as u64, block_size) as usize;
        let nt = redux_segment_static_table_count(nb as u64, element_size, segment_blocks) as usize;
        if nt == 0 {
            return Err(Error::InvalidInput);
        }
        let cap = redux_segment_static_encode_bound(&cp, data.len() as u64, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        let mut cum = vec![0u32; nt * 258];
        try!(status(redux_segment_static_encode_blocks_crc(&cp, total, data.as_ptr(), data.len() as u64, block_size, element_size,
                                                           segment_blocks, cum.as_mut_ptr(), out.as_mut_ptr(), cap as u64,
                                                           offs.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs, cum))
    }
}

/// Inverse of `compress_blocks_segment_static`: the original `len` bytes.
pub fn decompress_blocks_segment_static(streams: &[u8], offsets: &[u64], cum: &[u32], len: u64, block_size: u32,
                                        element_size: u32, segment_blocks: u32, p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || cum.len() % 258 != 0 || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    unsafe {
        if offsets.len() as u64 != redux_block_count(len, block_size) + 1 {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; if len == 0 { 1 } else { len as usize }];
        let mut sizes = vec![0u32; offsets.len() - 1];
        try!(status(redux_segment_static_decode_blocks_crc(&cp, cum.as_ptr(), (cum.len() / 258) as u64, streams.as_ptr(),
                                                           offsets.as_ptr(), len, block_size, element_size, segment_blocks,
                                                           out.as_mut_ptr(), sizes.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())));
        out.truncate(len as usize);
        Ok(out)
    }
}

/// Many independent inputs in ONE launch -- what the reference's corpus harness does file by file
/// (tests/corpora.rs:32-85).  Every input is cut into blocks of `block_size` on its own (ragged tail per
/// input, an empty input is one empty block); blocks are numbered input by input.  Returns the dense
/// streams, `nblocks + 1` offsets and, per input, the number of its first block (`inputs.len() + 1`
/// entries).  Block streams equal those of `compress_blocks` called once per input.
pub fn compress_blocks_v(inputs: &[&[u8]], block_size: u32, p: &Parameters) -> Result<(Vec<u8>, Vec<u64>, Vec<u64>)> {
    if block_size == 0 || inputs.is_empty() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    let lens: Vec<u64> = inputs.iter().map(|x| x.len() as u64).collect();
    let mut offs_in = vec![0u64; inputs.len()];
    let mut flat = Vec::with_capacity(lens.iter().sum::<u64>() as usize);
    let mut first = vec![0u64; inputs.len() + 1];
    for (i, x) in inputs.iter().enumerate() {
        offs_in[i] = flat.len() as u64;
        flat.extend_from_slice(x);
        first[i + 1] = first[i] + unsafe { redux_block_count(lens[i], block_size) };
    }
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count_v(lens.as_ptr(), lens.len() as u64, block_size) as usize;
        let cap = nb * redux_encode_slot_bytes(&cp, block_size) as usize;
        let mut out = vec![0u8; cap];
        let mut offs = vec![0u64; nb + 1];
        try!(status(redux_encode_blocks_v(&cp, flat.as_ptr(), offs_in.as_ptr(), lens.as_ptr(), lens.len() as u64, block_size,
                                          out.as_mut_ptr(), cap as u64, offs.as_mut_ptr(), ptr::null_mut())));
        out.truncate(offs[nb] as usize);
        Ok((out, offs, first))
    }
}

/// Inverse of `compress_blocks_v`: `lengths[i]` is the decoded size of input `i`; returns the inputs back to back
/// (input `i` at the sum of the lengths before it).
pub fn decompress_blocks_v(streams: &[u8], offsets: &[u64], lengths: &[u64], block_size: u32, p: &Parameters) -> Result<Vec<u8>> {
    if block_size == 0 || lengths.is_empty() || offsets.is_empty() || offsets[offsets.len() - 1] as usize > streams.len() {
        return Err(Error::InvalidInput);
    }
    let cp = c_params(p);
    let mut out_off = vec![0u64; lengths.len()];
    for i in 1..lengths.len() {
        out_off[i] = out_off[i - 1] + lengths[i - 1];
    }
    let total = (out_off[lengths.len() - 1] + lengths[lengths.len() - 1]) as usize;
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let nb = redux_block_count_v(lengths.as_ptr(), lengths.len() as u64, block_size) as usize;
        if nb + 1 != offsets.len() {
            return Err(Error::InvalidInput);
        }
        let mut out = vec![0u8; std::cmp::max(total, 1)];
        let mut sizes = vec![0u32; nb];
        try!(status(redux_decode_blocks_v(&cp, streams.as_ptr(), offsets.as_ptr(), out.as_mut_ptr(), out_off.as_ptr(),
                                          lengths.as_ptr(), lengths.len() as u64, block_size, sizes.as_mut_ptr(), ptr::null_mut())));
        out.truncate(total);
        Ok(out)
    }
}

/// Same signature shape and same bytes as `redux::compress` (src/lib.rs:102-109) with an
/// `AdaptiveTreeModel`: the whole stream is ONE block, coded by one GPU lane.  Correct, serial;
/// `compress_blocks` is the accelerated path.
pub fn compress(istream: &mut io::Read, ostream: &mut io::Write, p: &Parameters) -> Result<(u64, u64)> {
    let mut data = Vec::new();
    try!(istream.read_to_end(&mut data).map_err(Error::IoError));
    let cp = c_params(p);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        let bs = if data.is_empty() { 1 } else { data.len() as u32 };
        let cap = redux_encode_bound(&cp, data.len() as u64, bs) as usize;
        let mut out = vec![0u8; cap];
        let (mut bi, mut bo) = (0u64, 0u64);
        try!(status(redux_compress(&cp, data.as_ptr(), data.len() as u64, out.as_mut_ptr(), cap as u64, &mut bi, &mut bo)));
        try!(ostream.write_all(&out[..bo as usize]).map_err(Error::IoError));
        Ok((bi, bo))
    }
}

/// `redux::decompress` (src/lib.rs:113-120).  The reference writes to an unbounded `io::Write`;
/// the C ABI wants a capacity, so the buffer grows (x8) until the stream fits or the ABI's
/// one-block limit is reached.  Returns (compressed bytes the reader fetched, bytes written).
pub fn decompress(istream: &mut io::Read, ostream: &mut io::Write, p: &Parameters) -> Result<(u64, u64)> {
    const LIMIT: usize = 0xFFFF_FF00;
    let mut data = Vec::new();
    try!(istream.read_to_end(&mut data).map_err(Error::IoError));
    let cp = c_params(p);
    let mut cap = std::cmp::max(64 * data.len(), 1 << 20);
    unsafe {
        try!(status(redux_device_supports(&cp)));
        loop {
            cap = std::cmp::min(cap, LIMIT);
            let mut out = vec![0u8; cap];
            let (mut bi, mut bo) = (0u64, 0u64);
            let st = redux_decompress(&cp, data.as_ptr(), data.len() as u64, out.as_mut_ptr(), cap as u64, &mut bi, &mut bo);
            if st == 4 && cap < LIMIT {
                cap *= 8;
                continue;
            }
            try!(status(st));
            try!(ostream.write_all(&out[..bo as usize]).map_err(Error::IoError));
            return Ok((bi, bo));
        }
    }
}
