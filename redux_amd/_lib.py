"""ctypes loader of the C ABI declared in include/redux_hip.h.

There is no fallback of any kind: if libredux_hip.so is missing or a symbol is absent this
module raises, and every public function of redux_amd fails with it.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# The product library, in-tree.  REDUX_LIB names another build to load instead: how the A/B tools (tools/run_variants.sh,
# tools/small_grid.py ...) time a variant without ever overwriting the product library (an interrupted run used to leave
# a foreign library in its place that needs_build() would not replace).
LIB_PATH = os.environ.get("REDUX_LIB") or os.path.join(HERE, "libredux_hip.so")

OK, EOF, INVALID_INPUT, IO_ERROR, OUTPUT_TOO_SMALL, UNSUPPORTED = 0, 1, 2, 3, 4, 5


class Params(C.Structure):
    _fields_ = [("symbol_bits", C.c_uint32), ("freq_bits", C.c_uint32), ("code_bits", C.c_uint32)]


_PP = C.POINTER(Params)
_V = C.c_void_p
_U64 = C.c_uint64
_U32 = C.c_uint32

# name -> (restype, argtypes): exactly the declarations of include/redux_hip.h
SIGNATURES = {
    "redux_version": (C.c_char_p, []),
    "redux_source_hash": (C.c_char_p, []),
    "redux_encode_kernel_name": (C.c_char_p, [_PP, _V, _U64, _U32]),
    "redux_encode_kernel_name_ws": (C.c_char_p, [_PP, _V, _U64, _U32, _U64]),
    "redux_decode_kernel_name": (C.c_char_p, [_PP, _V, _U32]),
    "redux_decode_kernel_name_n": (C.c_char_p, [_PP, _V, _U32, _U64]),
    "redux_decode_kernel_name_table": (C.c_char_p, [_PP, _U32, _U64]),
    "redux_static_encode_kernel_name": (C.c_char_p, [_PP, C.POINTER(_U32), _U64, _U32]),
    "redux_static_decode_kernel_name": (C.c_char_p, [_PP, C.POINTER(_U32), _U64]),
    "redux_debug_rcp_check": (C.c_int, [_U64, _U64, C.POINTER(C.c_double)]),
    "redux_debug_role_book": (C.c_int, [_PP, _U64, _U32, C.POINTER(_U64), C.POINTER(_U64)]),
    "redux_debug_compact_tile_rows": (C.c_int, [_U32]),
    "redux_params_check": (C.c_int, [_U32, _U32, _U32]),
    "redux_device_supports": (C.c_int, [_PP]),
    "redux_block_count": (_U64, [_U64, _U32]),
    "redux_encode_slot_bytes": (_U64, [_PP, _U32]),
    "redux_encode_bound": (_U64, [_PP, _U64, _U32]),
    "redux_encode_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_decode_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_encode_blocks": (C.c_int, [_PP, _V, _U64, _U32, _V, _U64, _V, _V]),
    "redux_decode_blocks": (C.c_int, [_PP, _V, _V, _U64, _U32, _V, _U64, _V, _V]),
    "redux_block_count_v": (_U64, [_V, _U64, _U32]),
    "redux_block_table_v": (_U64, [_V, _V, _U64, _U32, _V]),
    "redux_encode_blocks_v": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _V, _U64, _V, _V]),
    "redux_decode_blocks_v": (C.c_int, [_PP, _V, _V, _V, _V, _V, _U64, _U32, _V, _V]),
    "redux_encode_blocks_v_dev": (C.c_int, [_PP, _V, _U64, _V, _U64, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_blocks_v_dev": (C.c_int, [_PP, _V, _V, _V, _U64, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_compress": (C.c_int, [_PP, _V, _U64, _V, _U64, C.POINTER(_U64), C.POINTER(_U64)]),
    "redux_decompress": (C.c_int, [_PP, _V, _U64, _V, _U64, C.POINTER(_U64), C.POINTER(_U64)]),
    "redux_host_release": (C.c_int, []),
    "redux_host_set_devices": (C.c_int, [_V, _U32]),
    "redux_host_chunk_plan": (C.c_int, [_U64, _U32, _U32, C.c_int, C.POINTER(_U64), C.POINTER(_U64)]),
    "redux_host_set_chunk_bytes": (C.c_int, [_U64, _U64]),
    "redux_host_allocations": (_U64, []),
    "redux_host_resident_bytes": (_U64, []),
    "redux_host_trace": (_U64, [C.POINTER(C.c_double), _U64]),
    "redux_encode_blocks_dev": (C.c_int, [_PP, _V, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_blocks_dev": (C.c_int, [_PP, _V, _V, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_slots_dev": (C.c_int, [_PP, _V, _U64, _U32, _V, _V, _U64, _V]),
    "redux_compact_slots_dev": (C.c_int, [_PP, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_static_table_check": (C.c_int, [_PP, C.POINTER(_U32)]),
    "redux_static_encode_bound": (_U64, [_PP, _U64, _U32]),
    "redux_static_encode_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_static_encode_blocks_dev": (C.c_int, [_PP, C.POINTER(_U32), _V, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_static_decode_blocks_dev": (C.c_int, [_PP, C.POINTER(_U32), _V, _V, _U64, _U32, _V, _U64, _V, _V, _V, _V]),
    "redux_static_table_from_counts": (C.c_int, [_PP, _V, _U32, _V]),
    "redux_histogram_workspace_bytes": (_U64, [_U64]),
    "redux_histogram_dev": (C.c_int, [_V, _U64, _V, _V, _U64, _V]),
    "redux_static_table_dev": (C.c_int, [_PP, _V, _U32, _V, _V]),
    "redux_static_table": (C.c_int, [_PP, _V, _U64, _U32, _V]),
    "redux_static_encode_blocks": (C.c_int, [_PP, _V, _V, _U64, _U32, _V, _U64, _V, _V]),
    "redux_static_decode_blocks": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _V, _U64, _V, _V]),
    "redux_crc32_blocks_dev": (C.c_int, [_V, _U64, _U32, _V, _V]),
    "redux_crc32_sizes_dev": (C.c_int, [_V, _U64, _U32, _V, _V, _V]),
    "redux_crc32_combine": (_U32, [_U32, _U32, _U64]),
    "redux_crc32_blocks": (C.c_int, [_V, _U64, _U32, _V]),
    "redux_encode_blocks_crc": (C.c_int, [_PP, _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_crc": (C.c_int, [_PP, _V, _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_static_encode_blocks_crc": (C.c_int, [_PP, C.POINTER(_U32), _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_static_decode_blocks_crc": (C.c_int, [_PP, C.POINTER(_U32), _V, _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_encode_stored_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_stored_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_encode_stored_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V, _U64, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_stored_dev": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_stored": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V, _U64, _V, _V, _V, _V]),
    "redux_decode_blocks_stored": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V]),
    "redux_plane_static_table_check": (C.c_int, [_PP, _V, _U32]),
    "redux_plane_static_total": (_U32, [_V, _U32]),
    "redux_plane_static_tables_from_counts": (C.c_int, [_PP, _V, _U32, _U32, _V]),
    "redux_plane_histogram_workspace_bytes": (_U64, [_U64]),
    "redux_plane_histogram_dev": (C.c_int, [_V, _U64, _U32, _U32, _V, _V, _U64, _V]),
    "redux_plane_static_tables_dev": (C.c_int, [_PP, _V, _U32, _U32, _V, _V]),
    "redux_plane_static_tables": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V]),
    "redux_plane_static_encode_bound": (_U64, [_PP, _U64, _U32]),
    "redux_plane_static_encode_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_plane_static_decode_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_plane_static_encode_dev": (C.c_int, [_PP, _V, _U32, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_plane_static_decode_dev": (C.c_int, [_PP, _V, _U32, _V, _V, _U64, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_plane_static_encode_blocks_crc": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V]),
    "redux_plane_static_decode_blocks_crc": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _U32, _V, _V, _V, _V]),
    "redux_plane_static_encode_kernel_name": (C.c_char_p, [_PP, _U32, _U64, _U32, _U32]),
    "redux_plane_static_decode_kernel_name": (C.c_char_p, [_PP, _U32, _U64, _U32]),
    "redux_segment_static_table_count": (_U64, [_U64, _U32, _U32]),
    "redux_segment_static_table_check": (C.c_int, [_PP, _V, _U64, _U64, _U32, _U32]),
    "redux_segment_static_total": (_U32, [_V, _U64]),
    "redux_segment_static_tables_from_counts": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V]),
    "redux_segment_histogram_dev": (C.c_int, [_V, _U64, _U32, _U32, _U32, _V, _V]),
    "redux_segment_static_tables_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V, _V]),
    "redux_segment_static_encode_bound": (_U64, [_PP, _U64, _U32]),
    "redux_segment_static_encode_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_segment_static_decode_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_segment_static_build_encode_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32, _U32]),
    "redux_segment_static_encode_dev": (C.c_int, [_PP, _V, _U32, _V, _U64, _U32, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_segment_static_build_encode_dev": (C.c_int, [_PP, _U32, _V, _U64, _U32, _U32, _U32, _V, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_segment_static_decode_dev": (C.c_int, [_PP, _V, _U32, _V, _V, _U64, _U32, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_segment_static_encode_blocks_crc": (C.c_int, [_PP, _U32, _V, _U64, _U32, _U32, _U32, _V, _V, _U64, _V, _V, _V]),
    "redux_segment_static_decode_blocks_crc": (C.c_int, [_PP, _V, _U64, _V, _V, _U64, _U32, _U32, _U32, _V, _V, _V, _V]),
    "redux_segment_static_encode_kernel_name": (C.c_char_p, [_PP, _U32, _U64, _U32, _U32, _U32]),
    "redux_segment_static_decode_kernel_name": (C.c_char_p, [_PP, _U32, _U64, _U32, _U32]),
    "redux_context_static_table_check": (C.c_int, [_PP, _V]),
    "redux_context_static_total": (_U32, [_V]),
    "redux_context_static_tables_from_counts": (C.c_int, [_PP, _V, _U32, _V]),
    "redux_context_histogram_dev": (C.c_int, [_V, _U64, _U32, _V, _V]),
    "redux_context_static_tables_dev": (C.c_int, [_PP, _V, _U32, _V, _V]),
    "redux_context_static_tables": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V]),
    "redux_context_static_encode_bound": (_U64, [_PP, _U64, _U32]),
    "redux_context_static_encode_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_context_static_decode_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_context_static_encode_dev": (C.c_int, [_PP, _V, _U32, _V, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_context_static_decode_dev": (C.c_int, [_PP, _V, _U32, _V, _V, _U64, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_context_static_encode_blocks_crc": (C.c_int, [_PP, _V, _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_context_static_decode_blocks_crc": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _V, _U64, _V, _V, _V]),
    "redux_context_static_encode_kernel_name": (C.c_char_p, [_PP, _U32, _U64, _U32]),
    "redux_context_static_decode_kernel_name": (C.c_char_p, [_PP, _U32, _U64]),
    "redux_adaptive_cost_from_counts": (C.c_int, [_PP, _V, _U64, C.POINTER(C.c_double)]),
    "redux_table_cost_from_counts": (C.c_int, [_V, _V, _U64, C.POINTER(C.c_double)]),
    "redux_block_cost_dev": (C.c_int, [_PP, _V, _U64, _U32, _V, _V]),
    "redux_table_cost_dev": (C.c_int, [_V, _V, _U64, _V, _V]),
    "redux_layout_cost_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _V]),
    "redux_layout_cost_kernel_name": (C.c_char_p, [_U64, _U32, _U32]),
    "redux_layout_cost_kernel_name_at": (C.c_char_p, [_V, _U64, _U32, _U32]),
    "redux_lag_cost_block_count": (_U64, [_U64, _U32, _U32, _U32]),
    "redux_lag_cost_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _U32, _U32, _V, _V]),
    "redux_lag_cost_kernel_name": (C.c_char_p, [_U64, _U32, _U32]),
    "redux_lag_cost_kernel_name_at": (C.c_char_p, [_V, _U64, _U32, _U32]),
    # order estimates: the lag estimates for (lag, order) candidates
    "redux_lag_order_cost_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _V, _U32, _U32, _V, _V]),
    "redux_lag_order_cost_kernel_name": (C.c_char_p, [_U64, _U32, _U32]),
    "redux_lag_order_cost_kernel_name_at": (C.c_char_p, [_V, _U64, _U32, _U32]),
    # record estimates: the cost behind the record layout for (record size, delta) candidates
    "redux_record_cost_frame_step": (_U32, [_U64, _U32, _U32, _U32]),
    "redux_record_cost_block_count": (_U64, [_U64, _U32, _U32, _U32]),
    "redux_record_cost_dev": (C.c_int, [_PP, _V, _U64, _U32, _V, _V, _U32, _U32, _V, _V]),
    "redux_record_cost_kernel_name": (C.c_char_p, [_U64, _U32, _U32]),
    "redux_record_cost_kernel_name_at": (C.c_char_p, [_V, _U64, _U32, _U32]),
    # mixed layouts: a layout per unit of 8 blocks
    "redux_mixed_unit_count": (_U64, [_U64, _U32]),
    "redux_mixed_choose_dev": (C.c_int, [_V, _U64, _U32, _V, _V, _V]),
    "redux_mixed_layout_dev": (C.c_int, [_V, _V, _U64, _U32, _V, C.c_int, _V]),
    "redux_encode_mixed_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_decode_mixed_workspace_bytes": (_U64, [_PP, _U64, _U32]),
    "redux_encode_mixed_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_mixed_dev": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_mixed": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_mixed": (C.c_int, [_PP, _V, _V, _V, _U64, _U32, _V, _V, _V, _V]),
    "redux_mixed_kernel_name": (C.c_char_p, [_U64, _U32, C.c_int]),
    "redux_mixed_kernel_name_at": (C.c_char_p, [_V, _V, _U64, _U32, C.c_int]),
    # range reads: the plan of the covered granules, and the segmented byte copy
    "redux_range_plan": (C.c_int, [_U64, _U32, _U64, _V, _V, _U64, _V, _V, C.POINTER(_U64), _V, C.POINTER(_U64)]),
    "redux_segment_copy_workspace_bytes": (_U64, [_V, _U64]),
    "redux_segment_tiles": (_U64, [_V, _U64, _V]),
    "redux_segment_copy_dev": (C.c_int, [_V, _U64, _V, _U64, _V, _U64, _V, _U64, _V]),
    "redux_segment_copy_kernel_name": (C.c_char_p, []),
    "redux_encode_blocks_planes": (C.c_int, [_PP, _V, _U64, _U32, _U32, _V, _U64, _V, _V]),
    "redux_decode_blocks_planes": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _V, _V, _V]),
    "redux_const_blocks_dev": (C.c_int, [_V, _U64, _U32, _V, _V]),
    "redux_encode_const_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_const_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_encode_const_dev": (C.c_int, [_PP, _V, _U64, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_const_dev": (C.c_int, [_PP, _V, _V, _V, _V, _U64, _U64, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_const": (C.c_int, [_PP, _V, _U64, _V, _U64, _U32, _U32, _V, _U64, _V, _V, _V, _V]),
    "redux_decode_blocks_const": (C.c_int, [_PP, _V, _V, _V, _V, _U64, _U64, _U32, _U32, _V, _V, _V, _V]),
    "redux_gen_iid_dev": (C.c_int, [_V, _U64, _U64, _U64, _V]),
    "redux_gen_zipf_dev": (C.c_int, [_V, _U64, _U64, _U64, _V]),
    "redux_zipf_thresholds": (C.POINTER(_U32), []),
}



def _family(infix, base, transform=None, blocks=None):
    """The eight entry points of a filter in front of the byte-plane layout (include/redux_hip.h): the check, the transform,
    the two workspace sizes, the `_dev` coder calls and the host-pointer ones.  base: they take a (base, base_len) pair
    behind their input.  The layout's own family names its transform and its host-pointer calls differently."""
    y = [_V, _U64] if base else []
    blocks = blocks or infix
    return {
        "redux_%s_check" % infix: (C.c_int, [_U32]),
        transform or "redux_%s_planes_dev" % infix: (C.c_int, [_V, *y, _V, _U64, _U32, _U32, C.c_int, _V]),
        "redux_encode_%s_workspace_bytes" % infix: (_U64, [_PP, _U64, _U32, _U32]),
        "redux_decode_%s_workspace_bytes" % infix: (_U64, [_PP, _U64, _U32, _U32]),
        "redux_encode_%s_dev" % infix: (C.c_int, [_PP, _V, _U64, *y, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
        "redux_decode_%s_dev" % infix: (C.c_int, [_PP, _V, _V, *y, _U64, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
        "redux_encode_blocks_%s" % blocks: (C.c_int, [_PP, _V, _U64, *y, _U32, _U32, _V, _U64, _V, _V, _V]),
        "redux_decode_blocks_%s" % blocks: (C.c_int, [_PP, _V, _V, *y, _U64, _U32, _U32, _V, _V, _V, _V]),
    }


SIGNATURES.update(_family("planes", False, transform="redux_planes_dev", blocks="planes_crc"))
for _infix, _base in (("delta", False), ("zigzag", False), ("base", True), ("base_sub", True)):
    SIGNATURES.update(_family(_infix, _base))
# the lagged delta filter: the zigzag family with the lag behind the element size (the workspace sizes take none)
SIGNATURES.update({
    "redux_lag_check": (C.c_int, [_U32, _U32]),
    "redux_lag_planes_dev": (C.c_int, [_V, _V, _U64, _U32, _U32, _U32, C.c_int, _V]),
    "redux_encode_lag_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_lag_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_encode_lag_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_lag_dev": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_lag": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_lag": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U32, _V, _V, _V, _V]),
})
# higher-order lagged differences: the lag family with the order behind the lag
SIGNATURES.update({
    "redux_lag_order_check": (C.c_int, [_U32, _U32, _U32]),
    "redux_lag_order_planes_dev": (C.c_int, [_V, _V, _U64, _U32, _U32, _U32, _U32, C.c_int, _V]),
    "redux_encode_lag_order_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_lag_order_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_encode_lag_order_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _U32, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_lag_order_dev": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U32, _U32, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_lag_order": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U32, _U32, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_lag_order": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U32, _U32, _V, _V, _V, _V]),
})
# the record layout: the lag family with (record size, delta flag) in place of (element size, lag)
SIGNATURES.update({
    "redux_record_check": (C.c_int, [_U32, C.c_int]),
    "redux_record_planes_dev": (C.c_int, [_V, _V, _U64, _U32, _U32, C.c_int, C.c_int, _V]),
    "redux_encode_record_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_record_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_encode_record_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, C.c_int, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_record_dev": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, C.c_int, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_record": (C.c_int, [_PP, _V, _U64, _U32, _U32, C.c_int, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_record": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, C.c_int, _V, _V, _V, _V]),
    "redux_host_chunk_plan_record": (C.c_int, [_U64, _U32, _U32, _U32, C.c_int, C.POINTER(_U64), C.POINTER(_U64)]),
    "redux_record_kernel_name": (C.c_char_p, [_U64, _U32, _U32, C.c_int]),
    "redux_record_kernel_name_at": (C.c_char_p, [_V, _V, _U64, _U32, _U32, C.c_int]),
    "redux_record_plan": (C.c_int, [_U64, _U32, _U32, C.c_int, C.c_int, _U32, C.POINTER(_U32)]),
})
# the snapshot-stride filter: the lag family with the stride, a u64, where the lag is; the transform takes a workspace in
# front of its stream and the decode workspace size takes the stride
SIGNATURES.update({
    "redux_stride_check": (C.c_int, [_U32, _U64]),
    "redux_stride_workspace_bytes": (_U64, [_U64, _U32, _U64]),
    "redux_stride_planes_dev": (C.c_int, [_V, _V, _U64, _U32, _U32, _U64, C.c_int, _V, _U64, _V]),
    "redux_encode_stride_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32]),
    "redux_decode_stride_workspace_bytes": (_U64, [_PP, _U64, _U32, _U32, _U64]),
    "redux_encode_stride_dev": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U64, _V, _U64, _V, _V, _V, _V, _U64, _V]),
    "redux_decode_stride_dev": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U64, _V, _V, _V, _V, _V, _U64, _V]),
    "redux_encode_blocks_stride": (C.c_int, [_PP, _V, _U64, _U32, _U32, _U64, _V, _U64, _V, _V, _V]),
    "redux_decode_blocks_stride": (C.c_int, [_PP, _V, _V, _U64, _U32, _U32, _U64, _V, _V, _V, _V]),
    "redux_stride_kernel_name": (C.c_char_p, [_U64, _U32, _U32, _U64, C.c_int, _V, _V]),
})

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m redux_amd.build` "
                "(there is no CPU fallback for the redux hot path)")
        # One HIP runtime per process: torch ships its own libamdhip64.so (SONAME
        # libamdhip64.so.7).  Loaded first, it satisfies this library's NEEDED entry, so both
        # share a runtime (and device pointers / streams are interchangeable).  Loaded second,
        # torch would bring a second runtime that cannot open the device.  A consumer without
        # torch (plain C/C++) gets the system ROCm runtime through the library's RUNPATH.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB
