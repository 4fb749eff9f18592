"""imageexperiments_amd -- MI355X (gfx950) drop-in for the CompressionLib tile-encode path of
mnesbit/ImageExperiments: host dictionary/quant/entropy code in C++, the quantized matching
pursuit as hand-written HIP, behind the C ABI of include/mpcodec.h.

Python here is plumbing only (ctypes binding, torch for device memory/streams/torch.distributed).
"""
from .api import (CompressionContext, MpcError, PatchStatistics, RatePoint, format_double, parse_qualities, quant_tables, assemble_streams, assemble_symbol_streams, assemble_symbol_streams_by_plan_indexed, calculate_psnr, changed_tiles, delta_pack_geometry, DeltaEncoder, PatchDecoder, patch_make, patch_info, patch_tiles, patch_index, patch_add_index, patch_strip_index, budget_lambda, budget_weights, budget_allocate, owed_tiles, budget_allocate_floor, budget_sweep, quality_pick, sse_for_psnr, RateInfo, BudgetResult, QualityResult, compose_container, container_index, container_index2, container_index_scan, container_info, index_aux, index_extend, index_info, index_version, window_chunks_by_index, parse_container_by_index, parse_container_window_by_index, parse_container_view_by_index, transcode_container, truncate_container, MpcRect, MpcView, create_compression_context,  # noqa: F401
                  decode_image, huffman_decode, huffman_encode, library_path, load_library, read_compressed,
                  run_length_decode, run_length_encode, write_compressed)

__all__ = ["CompressionContext", "MpcError", "PatchStatistics", "RatePoint", "format_double", "parse_qualities", "quant_tables", "assemble_streams", "assemble_symbol_streams", "assemble_symbol_streams_by_plan_indexed", "calculate_psnr", "changed_tiles", "delta_pack_geometry", "DeltaEncoder", "PatchDecoder", "patch_make", "patch_info", "patch_tiles", "patch_index", "patch_add_index", "patch_strip_index", "budget_lambda", "budget_weights", "budget_allocate", "owed_tiles", "budget_allocate_floor", "budget_sweep", "quality_pick", "sse_for_psnr", "RateInfo", "BudgetResult", "QualityResult", "compose_container", "container_index", "container_index2", "container_index_scan", "container_info", "index_aux", "index_extend", "index_info", "index_version", "window_chunks_by_index", "parse_container_by_index", "parse_container_window_by_index", "parse_container_view_by_index", "transcode_container", "truncate_container", "MpcRect", "MpcView", "create_compression_context",
           "decode_image", "huffman_decode", "huffman_encode", "library_path", "load_library", "read_compressed",
           "run_length_decode", "run_length_encode", "write_compressed"]
