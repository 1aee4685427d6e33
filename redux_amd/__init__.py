"""redux_amd -- MI355X-native block coder behind peterbudai/redux's compress/decompress.

Host-side mirror of the reference's public surface (src/lib.rs, src/model/mod.rs) on top of
the C ABI in include/redux_hip.h.  All coding runs in hand-written gfx950 kernels; nothing
here computes a bitstream on the CPU.
"""
from .api import (  # noqa: F401
    Error, Eof, InvalidInput, IoError, OutputTooSmall, Unsupported,
    Parameters, AdaptiveTreeModel, StaticModel, PlaneStaticModel, static_table, static_table_from_counts, plane_static_tables,
    compress, decompress, compress_blocks, decompress_blocks, compress_blocks_v, decompress_blocks_v, block_table_v, BLOCK_DTYPE, BLOCK_IDLE,
    host_set_devices, host_chunk_plan, host_set_chunk_bytes,
    DeviceEncoder, DeviceDecoder, DeviceStaticCoder, DevicePlaneStaticCoder, planes, delta_planes, zigzag_planes, base_planes, base_sub_planes, constant_blocks, gen_iid, gen_zipf, zipf_thresholds, version,
    crc32_blocks, crc32_combine, STORE_RATIO,
    ContextStaticModel, context_static_tables, context_static_tables_from_counts, DeviceContextStaticCoder,
    SegmentStaticModel, segment_static_tables, segment_static_tables_from_counts, default_segment_blocks, DeviceSegmentStaticCoder,
    MODELS, adaptive_cost_from_counts, table_cost_from_counts, block_cost, table_cost, estimate_candidates, estimate_payload,
    LAYOUTS, layout_index, layout_cost, estimate_layouts, BASE_OPS, estimate_base_ops,
    mixed_units, choose_unit_layouts, mixed_layout,
    lag_cost, estimate_lags, choose_lag,
    lag_order_cost, estimate_lag_orders, choose_lag_order,
    record_planes, record_kernel_name, record_plan, RECORD_MAX,
    stride_planes, stride_kernel_name,
    record_cost, estimate_records, choose_record, RECORD_COST_MAX,
    range_plan, segment_copy, segment_tiles, SEGMENT_DTYPE,
)
