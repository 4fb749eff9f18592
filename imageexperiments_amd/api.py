"""ctypes binding of libmpcodec.so (include/mpcodec.h) and a thin host-side mirror of the reference's
`compressed::` / `matching::` interface (CompressionLib/inc/CompressedImage.h, MatchingPursuit.h).

There is no CPU fallback: if the library is missing this module raises, and without a GPU the
encode entry points raise MpcError(MPC_ERR_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_K = 32
HIST_BINS = 8192

MPC_OK, MPC_ERR_ARGUMENT, MPC_ERR_NO_DEVICE, MPC_ERR_HIP, MPC_ERR_BITSTREAM, MPC_ERR_ALLOC = range(6)
MPC_INDEX_EXPANDED = 1                                              # `flags` of mpc_container_index2 and the ...indexed2 encoders


class MpcError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"mpcodec status {status}: {text}")
        self.status = status


def library_path():
    """In-tree library; MPCODEC_LIB selects another build of it (A/B timing of two kernel versions in one run)."""
    return os.environ.get("MPCODEC_LIB") or os.path.join(HERE, "lib", "libmpcodec.so")


_lib = None

_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)


class _IndexHeader(C.Structure):                     # mpc_index_header
    _fields_ = [("interval", C.c_int), ("n_streams", C.c_int), ("serial_only", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("K", C.c_int), ("block_size", C.c_int), ("container_bytes", C.c_size_t)]


class MpcRect(C.Structure):                          # mpc_rect
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class MpcView(C.Structure):                          # mpc_view
    _fields_ = [("rect", MpcRect), ("steps", C.c_int), ("scale_log2", C.c_int)]


class MpcPart(C.Structure):                          # mpc_part
    _fields_ = [("source", C.c_int), ("rect", MpcRect), ("x", C.c_int), ("y", C.c_int), ("rgb", C.c_void_p), ("row_stride", C.c_size_t)]


MPC_COMPOSE_DEVICE_PIXELS = 2                                       # `flags` of mpc_compose_indexed


class MpcDeltaInfo(C.Structure):                     # mpc_delta_info
    _fields_ = [("tiles", C.c_int), ("changed", C.c_int), ("key", C.c_int)]


MPC_DELTA_KEY, MPC_DELTA_DEVICE_PIXELS, MPC_DELTA_PACK_ALWAYS = 1, 2, 4   # `flags` of mpc_delta_encode
MPC_DELTA_PACK_ROWS = 64


class MpcPatchInfo(C.Structure):                     # struct mpc_patch_info
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("sequence", C.c_uint32), ("key", C.c_int), ("n", C.c_int), ("tiles", C.c_int),
                ("container_offset", C.c_size_t), ("container_bytes", C.c_size_t)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class MpcRateInfo(C.Structure):                      # mpc_rate_info
    _fields_ = [("tiles", C.c_int), ("changed", C.c_int), ("key", C.c_int), ("candidates", C.c_int), ("sent_tiles", C.c_int), ("owed", C.c_int),
                ("lambda_index", C.c_int), ("probes", C.c_int), ("all_bytes", C.c_size_t), ("sse", C.c_ulonglong)]


class MpcBudgetInfo(C.Structure):                    # mpc_budget_info
    _fields_ = [("lambda_index", C.c_int), ("probes", C.c_int), ("full_bytes", C.c_size_t), ("sse", C.c_ulonglong),
                ("full_sse", C.c_ulonglong), ("records", C.c_ulonglong), ("full_records", C.c_ulonglong)]


MPC_BUDGET_LAMBDAS = 256


class MpcQualityInfo(C.Structure):                   # mpc_quality_info
    _fields_ = [("lambda_index", C.c_int), ("full_bytes", C.c_size_t), ("sse", C.c_ulonglong), ("full_sse", C.c_ulonglong),
                ("min_sse", C.c_ulonglong), ("records", C.c_ulonglong), ("full_records", C.c_ulonglong), ("model_bits_256", C.c_ulonglong)]


def _parts(parts, device_pixels=False):
    """[(source, rect, x, y)] -> (MpcPart array, what must stay alive).  source: an int with rect = (x, y, width, height) or None = all
    of it; or pixels, rect None: an HxWx3 uint8 array (a strided view keeps its row stride), with device_pixels a
    (data_ptr, width, height, row_stride) tuple"""
    made, keep = (MpcPart * max(len(parts), 1))(), []                # never a null pointer: no parts is the call's to refuse
    for at, (source, rect, x, y) in zip(made, parts):
        at.x, at.y = int(x), int(y)
        if isinstance(source, (int, np.integer)):
            at.source = int(source)
            at.rect = MpcRect(*[int(v) for v in (rect or (0, 0, 0, 0))])
            continue
        if rect is not None:
            raise ValueError("a pixel part has no rectangle")
        at.source = -1
        if device_pixels:
            ptr, width, height, row_stride = source
            at.rgb, at.row_stride = int(ptr), int(row_stride)
        else:
            px = np.asarray(source)
            if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3:
                raise ValueError("pixels: an HxWx3 uint8 array")
            if px.size and (px.strides[2] != 1 or px.strides[1] != 3 or px.strides[0] < 3 * px.shape[1]):
                px = np.ascontiguousarray(px)
            keep.append(px)
            height, width = px.shape[:2]
            at.rgb, at.row_stride = px.ctypes.data, px.strides[0]
        at.rect = MpcRect(0, 0, int(width), int(height))
    return made, keep


def _view(view):
    """(rect, steps, scale_log2) with rect = (x, y, width, height), (0, 0, 0, 0) or None = the whole frame -> MpcView"""
    if isinstance(view, MpcView):
        return view
    rect, steps, scale_log2 = view
    return MpcView(MpcRect(*[int(v) for v in (rect or (0, 0, 0, 0))]), int(steps), int(scale_log2))


class _IndexStreamInfo(C.Structure):                 # mpc_index_stream_info
    _fields_ = [("mode", C.c_int), ("packed", C.c_int), ("m", C.c_uint32), ("n_coded", C.c_uint64), ("expect", C.c_uint64),
                ("wrapper_bit", C.c_uint64), ("end_bit", C.c_uint64), ("n_checkpoints", C.c_uint64)]


def load_library():
    """Load libmpcodec.so; raises (loudly) if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7). Loading
    # torch FIRST makes the dynamic linker bind libmpcodec.so's libamdhip64.so.7 dependency to that same copy;
    # the other order leaves two runtimes in the process and the second one sees no devices.
    import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m imageexperiments_amd.build` "
                          "(there is no CPU fallback for the hot path)")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.mpc_version.restype = C.c_char_p
    L.mpc_last_error.restype = C.c_char_p
    L.mpc_context_create.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(vp)]
    L.mpc_context_destroy.argtypes = [vp]
    for f in ("K", "block_size", "num_base", "detail_rows", "device", "max_waves"):
        getattr(L, "mpc_context_" + f).argtypes = [vp]
        getattr(L, "mpc_context_" + f).restype = C.c_int
    L.mpc_context_set_fast.argtypes = [vp, C.c_int]
    try:
        L.mpc_context_set_tile_encode_workgroups.argtypes = [vp, C.c_int]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    L.mpc_context_is_fast.argtypes = [vp]
    L.mpc_context_is_fast.restype = C.c_int
    L.mpc_context_get_quant.argtypes = [vp, _dp]
    L.mpc_context_set_quant.argtypes = [vp, _dp]
    L.mpc_context_get_dictionary.argtypes = [vp, _dp, _i32p, _dp, _dp, _dp]
    L.mpc_encode_tiles_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _dp,
                                          vp, vp, vp, vp, C.c_int, vp]
    L.mpc_encode_batch_device.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _dp,
                                          vp, vp, vp, vp, C.c_int, vp]
    L.mpc_encode_tiles.argtypes = [vp, _u8p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _dp,
                                   _u16p, vp, _dp, _u32p]
    L.mpc_histogram_device.argtypes = [vp, vp, vp, C.c_longlong, vp, vp]
    L.mpc_calc_mp.argtypes = [vp, C.c_int, _dp, _dp, vp, C.POINTER(C.c_int)]
    L.mpc_calc_mp_batch.argtypes = [vp, C.c_int, _dp, _dp, C.c_int, vp, _u16p, _dp, _u32p]
    L.mpc_reserve.argtypes = [vp, C.c_longlong]
    L.mpc_kernel_timing_enable.argtypes = [vp, C.c_int]
    L.mpc_kernel_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.mpc_kernel_counters_read.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    _bind_bitstream(L)
    _bind_debug(L)
    _lib = L
    return L


def _bind_debug(L):
    """The tests' entry points to the pursuit screen's tables (include/mpcodec.h, "test entry points")."""
    vp = C.c_void_p
    L.mpc_debug_copy_gram_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mpc_debug_gram_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.mpc_debug_copy_filter_tiles.argtypes = [vp, C.c_int, C.c_int, _u16p]
    L.mpc_filter_tiles.argtypes = [_dp, C.c_int, C.c_int, C.c_int, _u16p, _u8p]
    L.mpc_debug_screen_probe_device.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    try:
        L.mpc_debug_track_probe_device.argtypes = [vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp]
        L.mpc_debug_pair_scratch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise


def _bind_bitstream(L):
    """Entry points of the host entropy stage / container."""
    vp = C.c_void_p
    L.mpc_free.argtypes = [vp]
    L.mpc_write_compressed.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, C.c_size_t,
                                       C.POINTER(_u16p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_assemble_streams.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, vp,
                                       C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_assemble_planar_streams.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, vp,
                                       C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    _ullp = C.POINTER(C.c_ulonglong)
    for f in ("mpc_assemble_symbol_streams", "mpc_assemble_symbol_streams_by_plan"):
        getattr(L, f).argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_code_symbol_streams_device.argtypes = [vp, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                                 C.POINTER(C.c_int)]
    try:
        L.mpc_assemble_symbol_streams_by_plan_indexed.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.c_int,
                                                                  C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t)]
        L.mpc_code_symbol_streams_device_indexed.argtypes = [vp, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.c_int, C.POINTER(_u8p),
                                                             C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.mpc_encode_images_indexed.argtypes = [vp, C.POINTER(_u8p), C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(_u8p),
                                                C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t)]
        L.mpc_encode_images_indexed_device.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(_u8p),
                                                       C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t)]
        _u, _szp = C.c_uint, C.POINTER(C.c_size_t)
        L.mpc_assemble_symbol_streams_by_plan_indexed2.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.c_int, _u,
                                                                   C.POINTER(_u8p), _szp, C.POINTER(_u8p), _szp]
        L.mpc_code_symbol_streams_device_indexed2.argtypes = [vp, C.c_int, C.c_int, _dp, _u16p, _u16p, _ullp, C.c_int, _u, C.POINTER(_u8p),
                                                              _szp, C.POINTER(_u8p), _szp, C.POINTER(C.c_int)]
        L.mpc_encode_images_indexed2.argtypes = [vp, C.POINTER(_u8p), C.c_int, C.c_int, C.c_int, _dp, C.c_int, _u, C.POINTER(_u8p), _szp,
                                                 C.POINTER(_u8p), _szp]
        L.mpc_encode_images_indexed2_device.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, _dp, C.c_int, _u,
                                                        C.POINTER(_u8p), _szp, C.POINTER(_u8p), _szp]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    L.mpc_read_compressed.argtypes = [_u8p, C.c_size_t, C.POINTER(vp)]
    L.mpc_streams_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_streams_quant.argtypes = [vp, _u16p]
    L.mpc_streams_length.argtypes = [vp, C.c_int]
    L.mpc_streams_length.restype = C.c_size_t
    L.mpc_streams_copy.argtypes = [vp, C.c_int, _u16p]
    L.mpc_streams_free.argtypes = [vp]
    L.mpc_read_compressed_coded.argtypes = [_u8p, C.c_size_t, C.POINTER(vp)]
    L.mpc_streams_packed.argtypes = [vp, C.c_int]
    L.mpc_streams_expected.argtypes = [vp, C.c_int]
    L.mpc_streams_expected.restype = C.c_size_t
    L.mpc_container_info.argtypes = [_u8p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_decode_images.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(_u8p), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int)]
    L.mpc_decode_images_device.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_decode_image_device.argtypes = [vp, _u8p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_unpack_symbol_streams_device.argtypes = [vp, C.c_int, _u16p, _ullp, _u8p, _ullp, C.POINTER(_u16p), C.POINTER(C.c_size_t)]
    L.mpc_container_index.argtypes = [_u8p, C.c_size_t, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_container_index2.argtypes = [_u8p, C.c_size_t, C.c_int, C.c_uint, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_container_index_scan.argtypes = [_u8p, C.c_size_t, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int)]
    L.mpc_index_extend.argtypes = [_u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_index_version.argtypes = [_u8p, C.c_size_t]
    L.mpc_index_version.restype = C.c_int
    L.mpc_index_aux.argtypes = [_u8p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), _u16p, _u8p, _u16p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mpc_index_info.argtypes = [_u8p, C.c_size_t, C.POINTER(_IndexHeader)]
    L.mpc_index_stream.argtypes = [_u8p, C.c_size_t, C.c_int, C.POINTER(_IndexStreamInfo), C.POINTER(C.c_uint64), C.c_size_t]
    L.mpc_parse_container_by_index.argtypes = [_u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(_u16p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.mpc_container_index_device.argtypes = [vp, _u8p, C.c_size_t, C.c_int, C.c_uint, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.mpc_debug_container_index_device.argtypes = [vp, _u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                                   C.POINTER(C.c_int)]
    L.mpc_decode_images_scan.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(_u8p), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.mpc_decode_images_scan_device.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_int)]
    L.mpc_parse_container_device.argtypes = [vp, _u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(_u16p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    _rp = C.POINTER(MpcRect)
    _win = [_u8p, C.c_size_t, _u8p, C.c_size_t, _rp, C.c_uint, C.POINTER(_u16p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.mpc_parse_container_window_by_index.argtypes = _win
    L.mpc_parse_container_window_device.argtypes = [vp] + _win
    _chunks = [_u8p, C.c_size_t, _u8p, C.c_size_t, _rp, C.c_uint, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.mpc_window_chunks_by_index.argtypes = _chunks
    L.mpc_window_chunks_device.argtypes = [vp] + _chunks
    L.mpc_decode_regions_indexed.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), _rp, C.c_int,
                                             C.c_uint, C.POINTER(_u8p), C.POINTER(C.c_int)]
    L.mpc_decode_regions_indexed_device.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), _rp,
                                                    C.c_int, C.c_uint, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    _vwp = C.POINTER(MpcView)
    _vparse = [_u8p, C.c_size_t, _u8p, C.c_size_t, _vwp, C.c_uint, C.POINTER(_u16p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.mpc_truncate_container.argtypes = [_u8p, C.c_size_t, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_parse_container_view_by_index.argtypes = _vparse
    L.mpc_transcode_container.argtypes = [_u8p, C.c_size_t, _vwp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_transcode_views_indexed.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), _vwp, C.c_int,
                                              C.c_uint, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.mpc_crop_records_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, _rp, C.c_int, vp, vp, vp]
    L.mpc_crop_records_check.argtypes = [vp, vp]
    _pp = C.POINTER(MpcPart)
    L.mpc_compose_container.argtypes = [C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, _pp, C.c_int, C.c_int, C.c_int, C.POINTER(_u8p),
                                        C.POINTER(C.c_size_t)]
    L.mpc_paste_records_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, _rp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]
    L.mpc_compose_indexed.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, _pp, C.c_int,
                                      C.c_int, C.c_int, C.c_uint, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    _szp_ = C.POINTER(C.c_size_t)
    try:
        L.mpc_changed_tiles.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _i32p, C.POINTER(C.c_int)]
        L.mpc_delta_pack_geometry.argtypes = [C.c_longlong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _szp_, _szp_]
        L.mpc_tile_diff_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, vp]
        L.mpc_pack_tiles_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
        L.mpc_scatter_records_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp]
        L.mpc_delta_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.mpc_delta_destroy.argtypes = [vp]
        L.mpc_delta_destroy.restype = None
        L.mpc_delta_encode.argtypes = [vp, vp, C.c_size_t, _dp, C.c_uint, C.c_int, C.POINTER(_u8p), _szp_, C.POINTER(_u8p), _szp_,
                                       C.POINTER(MpcDeltaInfo)]
        L.mpc_delta_changed.argtypes = [vp, _i32p, C.c_int, C.POINTER(C.c_int)]
        _pip = C.POINTER(MpcPatchInfo)
        L.mpc_patch_make.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, _i32p, C.c_int, _u8p, C.c_size_t, C.POINTER(_u8p), _szp_]
        L.mpc_patch_info.argtypes = [_u8p, C.c_size_t, _pip]
        L.mpc_patch_tiles.argtypes = [_u8p, C.c_size_t, _i32p, C.c_int, C.POINTER(C.c_int)]
        L.mpc_delta_encode_patch.argtypes = [vp, vp, C.c_size_t, _dp, C.c_uint, C.POINTER(_u8p), _szp_, C.POINTER(MpcDeltaInfo)]
        L.mpc_unpack_tiles_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, vp]
        L.mpc_patch_decoder_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.mpc_patch_decoder_destroy.argtypes = [vp]
        L.mpc_patch_decoder_destroy.restype = None
        L.mpc_patch_apply.argtypes = [vp, _u8p, C.c_size_t, _pip]
        L.mpc_patch_frame_device.argtypes = [vp, C.POINTER(vp)]
        L.mpc_patch_read.argtypes = [vp, vp, C.c_size_t]
        L.mpc_patch_changed.argtypes = [vp, _i32p, C.c_int, C.POINTER(C.c_int)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_patch_index.argtypes = [_u8p, C.c_size_t, _szp_, _szp_]
        L.mpc_patch_make_indexed.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, _i32p, C.c_int, _u8p, C.c_size_t, _u8p, C.c_size_t,
                                             C.POINTER(_u8p), _szp_]
        L.mpc_patch_add_index.argtypes = [_u8p, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(_u8p), _szp_]
        L.mpc_patch_strip_index.argtypes = [_u8p, C.c_size_t, C.POINTER(_u8p), _szp_]
        L.mpc_delta_encode_patch_indexed.argtypes = [vp, vp, C.c_size_t, _dp, C.c_uint, C.c_int, C.c_size_t, C.POINTER(_u8p), _szp_,
                                                     C.POINTER(MpcDeltaInfo)]
        L.mpc_patch_last_route.argtypes = [vp]
        L.mpc_patch_last_route.restype = C.c_int
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    _u64p = C.POINTER(C.c_uint64)
    try:
        L.mpc_budget_lambda.argtypes = [C.c_int, _u64p]
        L.mpc_budget_weights.argtypes = [_u8p, C.c_size_t, _u32p]
        L.mpc_budget_allocate.argtypes = [_u32p, _u16p, C.c_longlong, C.c_int, _u32p, C.c_int, _u8p, _u16p, _u64p]
        L.mpc_depth_profile_device.argtypes = [vp, vp, vp, _dp, vp, C.c_int, C.c_int, vp, vp]
        L.mpc_budget_allocate_device.argtypes = [vp, vp, vp, C.c_longlong, _u32p, C.c_int, vp, vp, vp, vp]
        for f in ("mpc_encode_image_budget", "mpc_encode_image_budget_device"):
            getattr(L, f).argtypes = [vp, vp, C.c_int, C.c_int, _dp, C.c_size_t, C.c_int, C.POINTER(_u8p), _szp_, C.POINTER(_u8p), _szp_, _u8p,
                                      C.POINTER(MpcBudgetInfo)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_budget_sweep.argtypes = [_u32p, _u16p, C.c_longlong, C.c_int, _u32p, _u64p]
        L.mpc_quality_pick.argtypes = [_u64p, C.c_uint64]
        L.mpc_quality_pick.restype = C.c_int
        L.mpc_sse_for_psnr.argtypes = [C.c_double, C.c_int, C.c_int, _u64p]
        L.mpc_budget_sweep_device.argtypes = [vp, vp, vp, C.c_longlong, _u32p, vp, vp]
        for f in ("mpc_encode_image_quality", "mpc_encode_image_quality_device"):
            getattr(L, f).argtypes = [vp, vp, C.c_int, C.c_int, _dp, C.c_ulonglong, C.c_int, C.POINTER(_u8p), _szp_, C.POINTER(_u8p), _szp_, _u8p,
                                      C.POINTER(MpcQualityInfo)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_owed_tiles.argtypes = [_u8p, _u16p, C.c_longlong, C.c_int, _i32p, C.c_int, _i32p, _u8p, _u8p, C.POINTER(C.c_int)]
        L.mpc_budget_allocate_floor.argtypes = [_u32p, _u16p, _u8p, _u8p, C.c_longlong, C.c_int, _u32p, C.c_int, _u8p, _u16p, _u8p, _u64p]
        L.mpc_owed_tiles_device.argtypes = [vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp, vp]
        L.mpc_gather_records_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.mpc_budget_allocate_floor_device.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, _u32p, C.c_int, vp, vp, vp, vp, vp]
        L.mpc_delta_encode_patch_budget.argtypes = [vp, vp, C.c_size_t, _dp, C.c_uint, C.c_size_t, C.POINTER(_u8p), _szp_, C.POINTER(MpcRateInfo)]
        L.mpc_delta_sent.argtypes = [vp, _u8p, C.c_int, C.POINTER(C.c_int)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_budget_allocate_emphasis.argtypes = [_u32p, _u16p, _u8p, C.c_longlong, C.c_int, _u32p, C.c_int, _u8p, _u16p, _u64p]
        L.mpc_budget_sweep_emphasis.argtypes = [_u32p, _u16p, _u8p, C.c_longlong, C.c_int, _u32p, _u64p]
        L.mpc_budget_allocate_floor_emphasis.argtypes = [_u32p, _u16p, _u8p, _u8p, _u8p, _i32p, C.c_longlong, C.c_longlong, C.c_int, _u32p,
                                                         C.c_int, _u8p, _u16p, _u8p, _u64p]
        L.mpc_emphasis_from_mask.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _u8p]
        L.mpc_budget_allocate_emphasis_device.argtypes = [vp, vp, vp, vp, C.c_longlong, _u32p, C.c_int, vp, vp, vp, vp]
        L.mpc_budget_sweep_emphasis_device.argtypes = [vp, vp, vp, vp, C.c_longlong, _u32p, vp, vp]
        L.mpc_budget_allocate_floor_emphasis_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_longlong, C.c_longlong, _u32p, C.c_int, vp, vp,
                                                                vp, vp, vp]
        L.mpc_emphasis_from_mask_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp]
        for f in ("mpc_encode_image_budget_emphasis", "mpc_encode_image_budget_emphasis_device"):
            getattr(L, f).argtypes = [vp, vp, vp, C.c_int, C.c_int, _dp, C.c_size_t, C.c_int, C.POINTER(_u8p), _szp_, C.POINTER(_u8p), _szp_,
                                      _u8p, C.POINTER(MpcBudgetInfo)]
        for f in ("mpc_encode_image_quality_emphasis", "mpc_encode_image_quality_emphasis_device"):
            getattr(L, f).argtypes = [vp, vp, vp, C.c_int, C.c_int, _dp, C.c_ulonglong, C.c_int, C.POINTER(_u8p), _szp_, C.POINTER(_u8p), _szp_,
                                      _u8p, C.POINTER(MpcQualityInfo)]
        L.mpc_delta_set_emphasis.argtypes = [vp, _u8p, C.c_int]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_budget_allocate_group.argtypes = [_u32p, _u16p, _u8p, C.c_int, C.c_longlong, C.c_int, _u32p, C.c_int, _u8p, _u16p, _u64p]
        L.mpc_budget_sweep_group.argtypes = [_u32p, _u16p, _u8p, C.c_int, C.c_longlong, C.c_int, _u32p, _u64p]
        L.mpc_sse_for_psnr_group.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, _u64p]
        L.mpc_budget_allocate_group_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_longlong, _u32p, C.c_int, vp, vp, vp, vp]
        L.mpc_budget_sweep_group_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_longlong, _u32p, vp, vp]
        for f, target, info in (("mpc_encode_images_budget", C.c_size_t, MpcBudgetInfo), ("mpc_encode_images_quality", C.c_ulonglong, MpcQualityInfo)):
            for name in (f, f + "_device"):
                getattr(L, name).argtypes = [vp, C.POINTER(C.c_void_p), vp, C.c_int, C.c_int, C.c_int, _dp, target, C.c_int, C.POINTER(_u8p), _szp_,
                                             C.POINTER(_u8p), _szp_, _u8p, C.POINTER(info), C.POINTER(info)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    try:
        L.mpc_changed_tiles_tolerance.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint32, _i32p, C.POINTER(C.c_int),
                                                  _u32p]
        L.mpc_tile_diff_tolerance_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_uint32, vp, vp, vp, vp]
        L.mpc_delta_set_tolerance.argtypes = [vp, C.c_uint32]
        L.mpc_delta_tolerance.argtypes = [vp]
        L.mpc_delta_tolerance.restype = C.c_uint32
        L.mpc_delta_held.argtypes = [vp, C.POINTER(C.c_int), _u64p]
        L.mpc_delta_frame.argtypes = [vp, vp, C.c_size_t]
        L.mpc_delta_frame_device.argtypes = [vp, C.POINTER(vp)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    L.mpc_parse_container_view_device.argtypes = [vp] + _vparse
    L.mpc_decode_views_indexed.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), _vwp, C.c_int,
                                           C.c_uint, C.POINTER(_u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_decode_views_indexed_device.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), _vwp,
                                                  C.c_int, C.c_uint, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_decode_images_indexed.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int,
                                            C.POINTER(_u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_decode_images_indexed_device.argtypes = [vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int,
                                                   C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_huffman_encode.argtypes = [_u16p, C.c_size_t, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_huffman_decode.argtypes = [_u8p, C.c_size_t, C.POINTER(_u16p), C.POINTER(C.c_size_t)]
    L.mpc_rle_encode.argtypes = [_u16p, C.c_size_t, C.POINTER(_u16p), C.POINTER(C.c_size_t)]
    L.mpc_rle_decode.argtypes = [_u16p, C.c_size_t, C.POINTER(_u16p), C.POINTER(C.c_size_t)]
    L.mpc_encode_image.argtypes = [vp, _u8p, C.c_int, C.c_int, _dp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_encode_images.argtypes = [vp, C.POINTER(_u8p), C.c_int, C.c_int, C.c_int, _dp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    try:
        L.mpc_encode_images_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(_u8p), C.c_int, C.c_int, C.c_int, _dp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):
            raise
    L.mpc_encode_images_device.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, _dp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_records_to_container_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, _dp, vp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    try:
        L.mpc_interleave_stripe_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):             # an older build may be loaded for A/B timing only
            raise
    L.mpc_encode_image_device.argtypes = [vp, vp, C.c_int, C.c_int, _dp, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    L.mpc_container_job_begin.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, _dp, vp]
    L.mpc_container_job_tables.argtypes = [vp, C.c_int]
    L.mpc_container_job_collect.argtypes = [vp, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_size_t)]
    try:
        L.mpc_container_job_cancel.argtypes = [vp, C.c_int]
    except AttributeError:
        if not os.environ.get("MPCODEC_LIB"):
            raise
    L.mpc_decode_tiles_device.argtypes = [vp, vp, vp, _dp, C.c_int, C.c_int, vp, vp]
    L.mpc_decode_image.argtypes = [vp, _u8p, C.c_size_t, C.POINTER(_u8p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_patch_stats_create.argtypes = [vp, C.c_uint, C.POINTER(vp)]
    L.mpc_patch_stats_destroy.argtypes = [vp]
    L.mpc_patch_stats_destroy.restype = None
    L.mpc_patch_stats_add_image.argtypes = [vp, _u8p, C.c_int, C.c_int, C.c_int]
    L.mpc_patch_stats_read.argtypes = [vp, _dp]
    L.mpc_patch_stats_report.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.mpc_format_double.argtypes = [C.c_double, C.c_char_p, C.c_int]
    L.mpc_psnr.argtypes = [_u8p, _u8p, C.c_int, C.c_int]
    L.mpc_psnr.restype = C.c_double
    _ullp_ = C.POINTER(C.c_ulonglong)
    L.mpc_quant_tables.argtypes = [C.c_int, C.c_int, C.c_double, _dp]
    L.mpc_distortion_device.argtypes = [vp, vp, vp, _dp, vp, C.c_int, C.c_int, vp, vp, vp]
    for f in ("mpc_rate_distortion", "mpc_rate_distortion_device"):
        getattr(L, f).argtypes = [vp, vp, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_size_t), _ullp_, _dp, C.POINTER(_u8p)]


def _take_bytes(L, p, n):
    out = C.string_at(p, n.value)
    L.mpc_free(C.cast(p, C.c_void_p))
    return out


class _Owned:
    """Keeps a buffer the library malloc'ed alive for the numpy view built on it, and frees it with mpc_free."""

    def __init__(self, L, p):
        self.L, self.p = L, C.cast(p, C.c_void_p)

    def __del__(self):
        if self.p:
            self.L.mpc_free(self.p)
            self.p = None


def _take_view(L, p, n):
    """The container as a read-only uint8 array ON the library's buffer (no copy; the array owns the buffer)."""
    if not n.value:
        L.mpc_free(C.cast(p, C.c_void_p))
        return np.zeros(0, np.uint8)
    owner = _Owned(L, p)
    buf = (C.c_uint8 * n.value).from_address(C.cast(p, C.c_void_p).value)
    buf._owner = owner                                   # the ctypes array is the base of the view: freed with it
    out = np.frombuffer(buf, np.uint8)
    out.flags.writeable = False
    return out


def _take_u16(L, p, n):
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint16)
    L.mpc_free(C.cast(p, C.c_void_p))
    return out


def _u16(a):
    a = np.ascontiguousarray(a, np.uint16)
    return a, a.ctypes.data_as(_u16p)


# -- host entropy stage (huffman:: / compressed:: free functions of the reference) -----------------------------
def huffman_encode(data):
    """huffman::huffmanEncode (Huffman.h:15) -> bytes."""
    L = load_library()
    a, p = _u16(data)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_huffman_encode(p, a.size, C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def huffman_decode(blob):
    """huffman::huffmanDecode (Huffman.h:18) -> uint16 array; raises MpcError(MPC_ERR_BITSTREAM) on invalid data."""
    L = load_library()
    buf = np.frombuffer(bytes(blob), np.uint8)
    out, n = _u16p(), C.c_size_t(0)
    _check(L.mpc_huffman_decode(buf.ctypes.data_as(_u8p), buf.size, C.byref(out), C.byref(n)))
    return _take_u16(L, out, n)


def run_length_encode(data):
    L = load_library()
    a, p = _u16(data)
    out, n = _u16p(), C.c_size_t(0)
    _check(L.mpc_rle_encode(p, a.size, C.byref(out), C.byref(n)))
    return _take_u16(L, out, n)


def run_length_decode(data):
    L = load_library()
    a, p = _u16(data)
    out, n = _u16p(), C.c_size_t(0)
    _check(L.mpc_rle_decode(p, a.size, C.byref(out), C.byref(n)))
    return _take_u16(L, out, n)


def write_compressed(width, height, K, block_size, quant, lengths, codes):
    """compressed::writeCompressed (CompressedImage.cpp:403): codes = 6K uint16 arrays, DC not yet differenced."""
    L = load_library()
    q = np.ascontiguousarray(quant, np.float64).reshape(3 * K)
    ln, lp = _u16(lengths)
    arrs = [np.ascontiguousarray(c, np.uint16) for c in codes]
    ptrs = (_u16p * (6 * K))(*[a.ctypes.data_as(_u16p) for a in arrs])
    sizes = (C.c_size_t * (6 * K))(*[a.size for a in arrs])
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_write_compressed(width, height, K, block_size, q.ctypes.data_as(_dp), lp, ln.size, ptrs, sizes,
                                  C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def assemble_streams(width, height, K, block_size, quant, counts, choices):
    """Host half of encodeImage: whole-frame records (tile t = tx*tiles_y + ty) -> container bytes."""
    L = load_library()
    q = np.ascontiguousarray(quant, np.float64).reshape(3 * K)
    cn, cp = _u16(counts)
    ch = np.ascontiguousarray(choices)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_assemble_streams(width, height, K, block_size, q.ctypes.data_as(_dp), cp, ch.ctypes.data_as(C.c_void_p),
                                  C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def assemble_planar_streams(width, height, K, block_size, quant, counts, planar):
    """assemble_streams for records in planar order, planar[ch, step, tile] (uint32 deltaId | intCoeff << 16)."""
    L = load_library()
    q = np.ascontiguousarray(quant, np.float64).reshape(3 * K)
    cn, cp = _u16(counts)
    pl = np.ascontiguousarray(planar)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_assemble_planar_streams(width, height, K, block_size, q.ctypes.data_as(_dp), cp, pl.ctypes.data_as(C.c_void_p),
                                         C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def _symbol_streams(K, streams):
    streams = [np.ascontiguousarray(x, np.uint16).ravel() for x in streams]
    assert len(streams) == 6 * K
    off = np.zeros(6 * K + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in streams])
    symbols = np.concatenate(streams) if int(off[-1]) else np.zeros(1, np.uint16)
    return np.ascontiguousarray(symbols, np.uint16), off


def assemble_symbol_streams(width, height, K, block_size, quant, counts, streams, by_plan=False):
    """Entropy stage + container on the host from streams that are already assembled: streams[6K] = codes[0..6K) (live symbols,
    the step-0 coefficient streams already difference coded), counts[3*tiles] = the lengths stream.
    by_plan: take the route of the device-side entropy stage (statistics -> tables and offsets -> codes) on the host."""
    L = load_library()
    q = np.ascontiguousarray(quant, np.float64).reshape(3 * K)
    cn, cp = _u16(counts)
    symbols, off = _symbol_streams(K, streams)
    out, n = _u8p(), C.c_size_t(0)
    fn = L.mpc_assemble_symbol_streams_by_plan if by_plan else L.mpc_assemble_symbol_streams
    _check(fn(width, height, K, block_size, q.ctypes.data_as(_dp), cp, symbols.ctypes.data_as(_u16p),
              off.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def assemble_symbol_streams_by_plan_indexed(width, height, K, block_size, quant, counts, streams, interval=0, expanded=False):
    """mpc_assemble_symbol_streams_by_plan_indexed: assemble_symbol_streams(by_plan=True) with the container's seek index recorded
    while the codes are written -> (container, index): index == container_index(container, interval), or None for streams
    that do not hold what `counts` implies (no parser accepts their container).  expanded: index version 2
    (mpc_assemble_symbol_streams_by_plan_indexed2 with MPC_INDEX_EXPANDED), index == container_index(container, interval,
    expanded=True)."""
    L = load_library()
    q = np.ascontiguousarray(quant, np.float64).reshape(3 * K)
    cn, cp = _u16(counts)
    symbols, off = _symbol_streams(K, streams)
    out, n, idx, ni = _u8p(), C.c_size_t(0), _u8p(), C.c_size_t(0)
    head = (width, height, K, block_size, q.ctypes.data_as(_dp), cp, symbols.ctypes.data_as(_u16p), off.ctypes.data_as(C.POINTER(C.c_ulonglong)),
            int(interval))
    tail = (C.byref(out), C.byref(n), C.byref(idx), C.byref(ni))
    if expanded:
        _check(L.mpc_assemble_symbol_streams_by_plan_indexed2(*head, MPC_INDEX_EXPANDED, *tail))
    else:
        _check(L.mpc_assemble_symbol_streams_by_plan_indexed(*head, *tail))
    return _take_bytes(L, out, n), (_take_bytes(L, idx, ni) if idx else None)


def container_info(blob):
    """mpc_container_info: the container's header alone -> (width, height, K, block_size); MpcError(MPC_ERR_BITSTREAM) for a
    header read_compressed refuses."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    W, H, K, bs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _check(L.mpc_container_info(buf.ctypes.data_as(_u8p), buf.size, C.byref(W), C.byref(H), C.byref(K), C.byref(bs)))
    return W.value, H.value, K.value, bs.value


def read_compressed(blob, coded=False):
    """compressed::readCompressed (CompressedImage.cpp:635) -> dict(W,H,K,bs,quant[3,K],lengths,codes[6K]).
    coded=True: the serial half alone (mpc_read_compressed_coded): codes as entropy-decoded -- still run-length packed where
    packed[i], the step-0 coefficient streams still difference coded -- plus packed[6K] and expect[6K]."""
    L = load_library()
    buf = np.frombuffer(bytes(blob), np.uint8)
    h = C.c_void_p()
    _check((L.mpc_read_compressed_coded if coded else L.mpc_read_compressed)(buf.ctypes.data_as(_u8p), buf.size, C.byref(h)))
    try:
        W, H, K, bs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(L.mpc_streams_info(h, C.byref(W), C.byref(H), C.byref(K), C.byref(bs)))
        quant = np.zeros((3, K.value), np.uint16)
        _check(L.mpc_streams_quant(h, quant.ctypes.data_as(_u16p)))

        def stream(i):
            a = np.zeros(L.mpc_streams_length(h, i), np.uint16)
            if a.size:
                _check(L.mpc_streams_copy(h, i, a.ctypes.data_as(_u16p)))
            return a
        out = dict(W=W.value, H=H.value, K=K.value, bs=bs.value, quant=quant, lengths=stream(-1),
                   codes=[stream(i) for i in range(6 * K.value)])
        if coded:
            out["packed"] = [bool(L.mpc_streams_packed(h, i)) for i in range(6 * K.value)]
            out["expect"] = [int(L.mpc_streams_expected(h, i)) for i in range(6 * K.value)]
        return out
    finally:
        L.mpc_streams_free(h)


def container_index(blob, interval=0, expanded=False):
    """mpc_container_index: the seek index of a container -> bytes.  interval: coded symbols per checkpoint, 32 ... 65536,
    0 = the library's default.  expanded: index version 2 (mpc_container_index2 with MPC_INDEX_EXPANDED), whose aux section lets a
    region decode cut run-length packed and step-0 coefficient streams too.  MpcError(MPC_ERR_BITSTREAM) for whatever
    read_compressed(coded=True) refuses."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    out, n = _u8p(), C.c_size_t(0)
    if expanded:
        _check(L.mpc_container_index2(buf.ctypes.data_as(_u8p), buf.size, int(interval), 1, C.byref(out), C.byref(n)))
    else:
        _check(L.mpc_container_index(buf.ctypes.data_as(_u8p), buf.size, int(interval), C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def container_index2(blob, interval=0, flags=0):
    """mpc_container_index2 as it is: flags 0 = container_index's bytes, 1 (MPC_INDEX_EXPANDED) = version 2"""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_container_index2(buf.ctypes.data_as(_u8p), buf.size, int(interval), int(flags), C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def container_index_scan(blob, interval=0, flags=0, segment_bits=0, window_bits=0):
    """mpc_container_index_scan: container_index2's blob without a serial parse of the container (step table, segment maps, chain
    and walk per stream, on the host: what the device scan computes) -> (index, route).  route 0 = the scan produced the blob,
    1 = it gave up and the serial builder answered.  segment_bits, window_bits: 0 = the defaults; other sizes are for tests."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    out, n, route = _u8p(), C.c_size_t(0), C.c_int(-1)
    _check(L.mpc_container_index_scan(buf.ctypes.data_as(_u8p), buf.size, int(interval), int(flags), int(segment_bits), int(window_bits),
                                      C.byref(out), C.byref(n), C.byref(route)))
    return _take_bytes(L, out, n), route.value


def index_extend(blob, index):
    """mpc_index_extend: the version-2 index container_index(blob, interval of `index`, expanded=True) gives, from a version-1
    index of the container (what the indexed encoders return), without the serial parse -> bytes.  An index that is refused is
    answered from the serial parse; a version-2 index comes back as a copy."""
    L = load_library()
    buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_index_extend(buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size, C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def index_version(index):
    """mpc_index_version: 1 or 2; 0 = not an index"""
    idx = np.frombuffer(index, np.uint8)
    return load_library().mpc_index_version(idx.ctypes.data_as(_u8p), idx.size)


def index_aux(index, stream):
    """mpc_index_aux: the aux entries of stream `stream` (0 = the lengths stream) of a version-2 index -> dict(out uint64, prev
    uint16, state uint8, dc uint16), one value per checkpoint; empty arrays for a version-1 index or a stream without entries."""
    L = load_library()
    idx = np.frombuffer(index, np.uint8)
    ptr = idx.ctypes.data_as(_u8p)
    n = C.c_size_t(0)
    _check(L.mpc_index_aux(ptr, idx.size, int(stream), None, None, None, None, 0, C.byref(n)))
    out, prev, state, dc = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint16), np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint16)
    if n.value:
        _check(L.mpc_index_aux(ptr, idx.size, int(stream), out.ctypes.data_as(C.POINTER(C.c_uint64)), prev.ctypes.data_as(_u16p),
                               state.ctypes.data_as(_u8p), dc.ctypes.data_as(_u16p), n.value, C.byref(n)))
    return dict(out=out, prev=prev, state=state, dc=dc)


def _window_chunks(fn, head, blob, index, rect, parse_all):
    buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
    _, _, K, _ = container_info(buf)
    rc = MpcRect(*[int(v) for v in rect])
    chunks = np.zeros((6 * K, 2), np.uint64)
    route = C.c_int(-1)
    _check(fn(*head, buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size, C.byref(rc), 1 if parse_all else 0,
              chunks.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(route)))
    return chunks, route.value


def window_chunks_by_index(blob, index, rect, parse_all=False):
    """mpc_window_chunks_by_index: the chunks [c0, c1) of each of the 6K streams the windowed parse reads for rect -> (chunks[6K, 2],
    route); route 1 = nothing is parsed by the index (all zero)."""
    return _window_chunks(load_library().mpc_window_chunks_by_index, (), blob, index, rect, parse_all)


def index_info(index):
    """mpc_index_info / mpc_index_stream: an index read back -> dict(interval, serial_only, nbytes, W, H, K, bs, streams), streams
    = one dict per stream (the lengths stream first): mode (0 Huffman, 1 Golomb), m, packed, n_coded, expect, wrapper_bit,
    end_bit, checkpoints (uint64 array).  MpcError(MPC_ERR_BITSTREAM) if it is not an index."""
    L = load_library()
    buf = np.frombuffer(index, np.uint8)
    ptr = buf.ctypes.data_as(_u8p)
    h = _IndexHeader()
    _check(L.mpc_index_info(ptr, buf.size, C.byref(h)))
    streams = []
    for j in range(h.n_streams):
        si = _IndexStreamInfo()
        _check(L.mpc_index_stream(ptr, buf.size, j, C.byref(si), None, 0))
        cp = np.zeros(si.n_checkpoints, np.uint64)
        _check(L.mpc_index_stream(ptr, buf.size, j, C.byref(si), cp.ctypes.data_as(C.POINTER(C.c_uint64)), cp.size))
        streams.append(dict(mode=si.mode, m=si.m, packed=bool(si.packed), n_coded=si.n_coded, expect=si.expect,
                            wrapper_bit=si.wrapper_bit, end_bit=si.end_bit, checkpoints=cp))
    return dict(interval=h.interval, serial_only=bool(h.serial_only), nbytes=h.container_bytes, W=h.width, H=h.height, K=h.K,
                bs=h.block_size, streams=streams)


def _window_parse(fn, head, buf, idx, rect, parse_all):
    _, _, K, _ = container_info(buf)
    rc = MpcRect(*[int(v) for v in rect])
    ranges = np.zeros((3 * K, 2), np.uint64)
    out, n, route = _u16p(), C.c_size_t(0), C.c_int(-1)
    _check(fn(*head, buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size, C.byref(rc), 1 if parse_all else 0, C.byref(out),
              C.byref(n), ranges.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(route)))
    return _take_u16(load_library(), out, n), ranges, route.value


def parse_container_window_by_index(blob, index, rect, parse_all=False):
    """mpc_parse_container_window_by_index: the windowed parse on the host for the pixel rectangle rect = (x, y, width, height) ->
    (symbols, ranges, route): the lengths stream whole, then of each of the 6K streams the expanded symbols [r0, r1) (run lengths
    undone, step-0 coefficients summed); ranges[3K, 2] = (r0, r1) per (channel, step); route 0 = by the index, 1 = the index
    was refused and the serial parse gave the result."""
    buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
    return _window_parse(load_library().mpc_parse_container_window_by_index, (), buf, idx, rect, parse_all)


def truncate_container(blob, steps):
    """mpc_truncate_container: the container cut to its first `steps` pursuit steps (the rate-scalable transcode) -> bytes: every
    length min(length, steps), the streams of steps at or above `steps` emptied, header, K and quantiser table kept.  steps >= K
    gives an encoder's container back as it is; steps < 1 is MpcError(MPC_ERR_ARGUMENT); MpcError(MPC_ERR_BITSTREAM) for whatever
    read_compressed refuses."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_truncate_container(buf.ctypes.data_as(_u8p), buf.size, int(steps), C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def transcode_container(blob, view):
    """mpc_transcode_container: view = (rect, steps, 0) of a container as a container -> bytes.  rect = (x, y, width, height) aligned
    to the container's tiles (a ragged right or bottom edge only where it is the frame's own), None = the whole frame; steps 0 = all.
    For an encoder's container the result is byte for byte the encode of the cropped pixels, truncated to `steps`; no pixels and no
    pursuit are involved.  MpcError(MPC_ERR_ARGUMENT) for a rectangle that is empty, outside the frame or not aligned, steps < 0,
    scale_log2 != 0; MpcError(MPC_ERR_BITSTREAM) for whatever read_compressed refuses and for a length above K."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)
    vw = _view(view)
    out, n = _u8p(), C.c_size_t(0)
    _check(L.mpc_transcode_container(buf.ctypes.data_as(_u8p), buf.size, C.byref(vw), C.byref(out), C.byref(n)))
    return _take_bytes(L, out, n)


def compose_container(blobs, parts, width, height):
    """mpc_compose_container: the container of a width x height frame from rectangles of containers -> bytes.  parts: [(source, rect, x,
    y)], rect = (x, y, width, height) of blobs[source] (None = all of it) landing at (x, y); applied in order, a later part wins a tile.
    Everything is aligned to the tiles; a ragged edge only where it is its source's own and lands on the destination's.  K, block size
    and quantiser values are blobs[0]'s and must be every blob's.  For containers encoded from pixels with one integral quantiser table
    the result is byte for byte the encode of the pasted pixels; no pixels and no pursuit are involved.  MpcError(MPC_ERR_ARGUMENT)
    "part N: ..." / "source N: ..." for bad geometry, an uncovered tile, a pixel part; MpcError(MPC_ERR_BITSTREAM) for a header that does
    not parse and for what read_compressed refuses of a source whose part owns a tile."""
    L = load_library()
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    n = len(bufs)
    ptrs, sizes = (_u8p * n)(*[b.ctypes.data_as(_u8p) for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs])
    made, keep = _parts(parts)
    out, nout = _u8p(), C.c_size_t(0)
    _check(L.mpc_compose_container(ptrs, sizes, n, made, len(parts), int(width), int(height), C.byref(out), C.byref(nout)))
    del keep
    return _take_bytes(L, out, nout)


def _pixel_rows(rgb):
    """an HxWx3 uint8 array whose pixels are contiguous within a row, as it is (strides[0] is its row stride: a window of a larger
    image, padded rows); anything else made contiguous"""
    rgb = np.asarray(rgb)
    if not (rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.strides[1:] == (3, 1) and rgb.strides[0] >= 3 * rgb.shape[1]):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("pixels: an HxWx3 uint8 array")
    return rgb


def changed_tiles(prev, cur, block_size=8):
    """mpc_changed_tiles: the tiles t = tx * tiles_y + ty of two equally sized HxWx3 uint8 frames that differ in any pixel byte, ascending
    (int32 array): the host's definition of the delta encoder's diff kernel.  Strided views keep their row strides; only pixel bytes
    are read."""
    L = load_library()
    prev, cur = _pixel_rows(prev), _pixel_rows(cur)
    if prev.shape != cur.shape:
        raise ValueError("frames must have the same size")
    H, W = cur.shape[:2]
    tiles = np.zeros(max(-(-W // max(block_size, 1)) * -(-H // max(block_size, 1)), 1), np.int32)
    n = C.c_int(0)
    _check(L.mpc_changed_tiles(prev.ctypes.data, prev.strides[0], cur.ctypes.data, cur.strides[0], W, H, int(block_size),
                               tiles.ctypes.data_as(_i32p), C.byref(n)))
    return tiles[:n.value].copy()


def changed_tiles_tolerance(prev, cur, tolerance, block_size=8):
    """mpc_changed_tiles_tolerance: the host's definition of the delta encoder's tolerant diff on two equally sized HxWx3 uint8 frames ->
    (the tiles whose summed squared byte difference exceeds `tolerance`, ascending, int32; every tile's sum, uint32; the composite the
    encoder keeps: `cur` in the listed tiles, `prev` in every other, HxWx3 uint8).  Strided views keep their row strides; only pixel
    bytes are read."""
    L = load_library()
    prev, cur = _pixel_rows(prev), _pixel_rows(cur)
    if prev.shape != cur.shape:
        raise ValueError("frames must have the same size")
    H, W = cur.shape[:2]
    bs = max(int(block_size), 1)
    tx, ty = -(-W // bs), -(-H // bs)
    tiles = np.zeros(max(tx * ty, 1), np.int32)
    sse = np.zeros(max(tx * ty, 1), np.uint32)
    n = C.c_int(0)
    _check(L.mpc_changed_tiles_tolerance(prev.ctypes.data, prev.strides[0], cur.ctypes.data, cur.strides[0], W, H, int(block_size),
                                         int(tolerance), tiles.ctypes.data_as(_i32p), C.byref(n), sse.ctypes.data_as(_u32p)))
    composite = np.array(prev)
    for t in tiles[:n.value]:
        cx, cy = divmod(int(t), ty)
        composite[cy * bs:cy * bs + bs, cx * bs:cx * bs + bs] = cur[cy * bs:cy * bs + bs, cx * bs:cx * bs + bs]
    return tiles[:n.value].copy(), sse[:tx * ty].copy(), composite


def delta_pack_geometry(n, rows=MPC_DELTA_PACK_ROWS):
    """mpc_delta_pack_geometry: the packed frame of n listed tiles with at most `rows` tile rows -> (R, C, stride, bytes): R x C whole
    tiles, listed tile j at tile (j // R, j % R), `stride` = 24 * C bytes between pixel rows."""
    R, Cc, stride, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    _check(load_library().mpc_delta_pack_geometry(int(n), int(rows), C.byref(R), C.byref(Cc), C.byref(stride), C.byref(nbytes)))
    return R.value, Cc.value, stride.value, nbytes.value


# DeltaEncoder.encode_patch's default index_min_bytes: the smallest container from which applying the version-2 patch won in the median
# at both measured frame sizes (profiles/patch_index.txt: 12134 bytes, 1 % of a 1920x1080 frame at K = 8; below it -- 8643 bytes at
# 4928x3264, K = 32, 1482 bytes at 1920x1080 -- the two versions are within 0.03 ms of each other and either wins from run to run)
PATCH_INDEX_MIN_BYTES = 12134


class DeltaEncoder:
    """mpc_delta: a session that encodes frames of one size one after the other and pursues only the tiles whose pixels changed since
    the last call.  Every container is byte for byte CompressionContext.encode_image of that frame.  `info` = (tiles, changed, key)
    of the last call."""

    def __init__(self, ctx, width, height):
        self.ctx, self.L = ctx, ctx.L                               # the session must go before its context
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _check(self.L.mpc_delta_create(ctx.h, self.width, self.height, C.byref(h)))
        self.h = h
        self.info = None

    def close(self):
        if getattr(self, "h", None):
            self.L.mpc_delta_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _encode(self, ptr, row_stride, quant, flags, index_interval):
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.ctx.K)
            qp = quant.ctypes.data_as(_dp)
        out, n, index, nindex, info = _u8p(), C.c_size_t(0), _u8p(), C.c_size_t(0), MpcDeltaInfo()
        _check(self.L.mpc_delta_encode(self.h, ptr, int(row_stride), qp, int(flags), -1 if index_interval is None else int(index_interval),
                                       C.byref(out), C.byref(n), C.byref(index), C.byref(nindex), C.byref(info)))
        self.info = (info.tiles, info.changed, info.key)
        blob = _take_bytes(self.L, out, n)
        return blob if index_interval is None else (blob, _take_bytes(self.L, index, nindex))

    def encode(self, rgb, quant=None, key=False, index_interval=None, pack_always=False):
        """mpc_delta_encode of a host frame (HxWx3 uint8; a strided view keeps its row stride) -> the container, or with index_interval
        (0 = the default interval) (container, container_index2(container, interval, expanded))."""
        rgb = _pixel_rows(rgb)
        if rgb.shape[:2] != (self.height, self.width):
            raise ValueError("the frame is not the session's size")
        flags = (MPC_DELTA_KEY if key else 0) | (MPC_DELTA_PACK_ALWAYS if pack_always else 0)
        return self._encode(rgb.ctypes.data, rgb.strides[0], quant, flags, index_interval)

    def encode_device(self, d_rgb, row_stride=0, quant=None, key=False, index_interval=None, pack_always=False):
        """The same for a frame in device memory: d_rgb an int from tensor.data_ptr(), row_stride bytes between rows (0 = 3 * width)."""
        flags = MPC_DELTA_DEVICE_PIXELS | (MPC_DELTA_KEY if key else 0) | (MPC_DELTA_PACK_ALWAYS if pack_always else 0)
        return self._encode(int(d_rgb), row_stride, quant, flags, index_interval)

    def changed(self):
        """mpc_delta_changed: the tiles the last call pursued, ascending (int32 array); a key frame's: every tile"""
        n = C.c_int(0)
        _check(self.L.mpc_delta_changed(self.h, None, 0, C.byref(n)))
        tiles = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.mpc_delta_changed(self.h, tiles.ctypes.data_as(_i32p), n.value, C.byref(n)))
        return tiles[:n.value]

    def _encode_patch(self, ptr, row_stride, quant, flags, index_interval=None, index_min_bytes=0):
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.ctx.K)
            qp = quant.ctypes.data_as(_dp)
        out, n, info = _u8p(), C.c_size_t(0), MpcDeltaInfo()
        if index_interval is None:
            _check(self.L.mpc_delta_encode_patch(self.h, ptr, int(row_stride), qp, int(flags), C.byref(out), C.byref(n), C.byref(info)))
        else:
            _check(self.L.mpc_delta_encode_patch_indexed(self.h, ptr, int(row_stride), qp, int(flags), int(index_interval), int(index_min_bytes),
                                                         C.byref(out), C.byref(n), C.byref(info)))
        self.info = (info.tiles, info.changed, info.key)
        return _take_bytes(self.L, out, n)

    def encode_patch(self, rgb, quant=None, key=False, pack_always=False, index_interval=None, index_min_bytes=PATCH_INDEX_MIN_BYTES):
        """mpc_delta_encode_patch of a host frame -> the patch (bytes): the changed tiles' list and the container of their packed frame,
        a key patch with the whole frame's container where every tile is listed, 40 bytes where none is.  With index_interval (0 = the
        default interval) mpc_delta_encode_patch_indexed: patch_add_index(that patch, index_interval, index_min_bytes), a version-2 patch
        whose container the receiver parses on the device.  index_min_bytes leaves patches with a smaller container at version 1: the
        default is the measured size from which version 2 applies faster (PATCH_INDEX_MIN_BYTES); 0 indexes every patch that has a
        container."""
        rgb = _pixel_rows(rgb)
        if rgb.shape[:2] != (self.height, self.width):
            raise ValueError("the frame is not the session's size")
        flags = (MPC_DELTA_KEY if key else 0) | (MPC_DELTA_PACK_ALWAYS if pack_always else 0)
        return self._encode_patch(rgb.ctypes.data, rgb.strides[0], quant, flags, index_interval, index_min_bytes)

    def encode_patch_device(self, d_rgb, row_stride=0, quant=None, key=False, pack_always=False, index_interval=None, index_min_bytes=PATCH_INDEX_MIN_BYTES):
        """The same for a frame in device memory: d_rgb an int from tensor.data_ptr(), row_stride bytes between rows (0 = 3 * width)."""
        flags = MPC_DELTA_DEVICE_PIXELS | (MPC_DELTA_KEY if key else 0) | (MPC_DELTA_PACK_ALWAYS if pack_always else 0)
        return self._encode_patch(int(d_rgb), row_stride, quant, flags, index_interval, index_min_bytes)


    def _encode_patch_budget(self, ptr, row_stride, budget, quant, flags):
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.ctx.K)
            qp = quant.ctypes.data_as(_dp)
        out, n, info = _u8p(), C.c_size_t(0), MpcRateInfo()
        _check(self.L.mpc_delta_encode_patch_budget(self.h, ptr, int(row_stride), qp, int(flags), int(budget), C.byref(out), C.byref(n),
                                                    C.byref(info)))
        self.info = (info.tiles, info.changed, info.key)
        return _take_bytes(self.L, out, n), RateInfo(info)

    def encode_patch_budget(self, rgb, budget, quant=None, key=False):
        """mpc_delta_encode_patch_budget of a host frame -> (the patch, at most `budget` bytes; RateInfo): the changed tiles, cut to the
        depths a multiplier found by bisection assigns them, and as many of the tiles sent thin before as the bytes left pay for."""
        rgb = _pixel_rows(rgb)
        if rgb.shape[:2] != (self.height, self.width):
            raise ValueError("the frame is not the session's size")
        return self._encode_patch_budget(rgb.ctypes.data, rgb.strides[0], budget, quant, MPC_DELTA_KEY if key else 0)

    def encode_patch_budget_device(self, d_rgb, budget, row_stride=0, quant=None, key=False):
        """The same for a frame in device memory: d_rgb an int from tensor.data_ptr(), row_stride bytes between rows (0 = 3 * width)."""
        return self._encode_patch_budget(int(d_rgb), row_stride, budget, quant, MPC_DELTA_DEVICE_PIXELS | (MPC_DELTA_KEY if key else 0))

    def set_emphasis(self, emphasis):
        """mpc_delta_set_emphasis: the emphasis map (uint8 per tile, 16 = neutral, 1 ... 64) that weighs every later encode_patch_budget
        until set again; None = none.  MpcError(MPC_ERR_ARGUMENT) for a map that is not the session's size; the session stays as it was."""
        if emphasis is None:
            _check(self.L.mpc_delta_set_emphasis(self.h, None, 0))
            return
        emphasis = np.ascontiguousarray(emphasis, np.uint8).reshape(-1)
        _check(self.L.mpc_delta_set_emphasis(self.h, emphasis.ctypes.data_as(_u8p), emphasis.size))

    def set_tolerance(self, tolerance):
        """mpc_delta_set_tolerance: from the next call on a tile is changed iff the summed squared difference of its pixel bytes against
        the pixels last sent exceeds `tolerance` (uint32; 0 = any differing byte, the default).  No key frame follows from it."""
        if not 0 <= int(tolerance) < 2**32:
            raise ValueError("tolerance: 0 ... 2^32 - 1")
        _check(self.L.mpc_delta_set_tolerance(self.h, int(tolerance)))

    @property
    def tolerance(self):
        """mpc_delta_tolerance"""
        return int(self.L.mpc_delta_tolerance(self.h))

    def held(self):
        """mpc_delta_held: (held, held_sse) of the last call -- the tiles that differed within the tolerance and the sum of their squared
        differences; held_sse / (3 * width * height) is the composite's mean squared error against the caller's frame"""
        n, sse = C.c_int(0), C.c_uint64(0)
        _check(self.L.mpc_delta_held(self.h, C.byref(n), C.byref(sse)))
        return n.value, sse.value

    def frame(self):
        """mpc_delta_frame: the composite the session keeps (HxWx3 uint8): what its last container encodes"""
        out = np.zeros((self.height, self.width, 3), np.uint8)
        _check(self.L.mpc_delta_frame(self.h, out.ctypes.data, 0))
        return out

    def frame_device(self):
        """mpc_delta_frame_device: the composite's address in device memory (int), height rows of 3 * width bytes, valid until the next
        call"""
        p = C.c_void_p()
        _check(self.L.mpc_delta_frame_device(self.h, C.byref(p)))
        return p.value

    def sent(self):
        """mpc_delta_sent: the depth the receiver holds of each tile after the last budget call (uint8 per tile)"""
        n = C.c_int(0)
        _check(self.L.mpc_delta_sent(self.h, None, 0, C.byref(n)))
        depth = np.zeros(max(n.value, 1), np.uint8)
        _check(self.L.mpc_delta_sent(self.h, depth.ctypes.data_as(_u8p), n.value, C.byref(n)))
        return depth[:n.value]


class RateInfo:
    """mpc_rate_info's fields of one DeltaEncoder.encode_patch_budget call"""
    __slots__ = tuple(f for f, _ in MpcRateInfo._fields_)

    def __init__(self, info):
        for f, _ in MpcRateInfo._fields_:
            setattr(self, f, int(getattr(info, f)))

    def __repr__(self):
        return "RateInfo(" + ", ".join(f"{f}={getattr(self, f)}" for f in self.__slots__) + ")"


def patch_make(width, height, sequence, tiles, container, key=False, index=None):
    """mpc_patch_make: the only writer of a patch -> bytes.  key: `tiles` is not read (None will do) and the container is the whole
    frame's; else `tiles` ascending with the container of their packed frame, or empty with container None or b"".  index (bytes, not
    empty): mpc_patch_make_indexed, a version-2 patch with those bytes as its index section."""
    L = load_library()
    buf = np.frombuffer(container if container is not None else b"", np.uint8)
    listed = np.ascontiguousarray([] if tiles is None else tiles, np.int32)
    n = -(-int(width) // 8) * -(-int(height) // 8) if key else listed.size
    out, nbytes = _u8p(), C.c_size_t(0)
    if index is None:
        _check(L.mpc_patch_make(int(width), int(height), int(sequence), int(bool(key)), listed.ctypes.data_as(_i32p) if listed.size else None, n,
                                buf.ctypes.data_as(_u8p) if buf.size else None, buf.size, C.byref(out), C.byref(nbytes)))
    else:
        ix = np.frombuffer(index, np.uint8)
        _check(L.mpc_patch_make_indexed(int(width), int(height), int(sequence), int(bool(key)), listed.ctypes.data_as(_i32p) if listed.size else None,
                                        n, buf.ctypes.data_as(_u8p) if buf.size else None, buf.size, ix.ctypes.data_as(_u8p) if ix.size else None,
                                        ix.size, C.byref(out), C.byref(nbytes)))
    return _take_bytes(L, out, nbytes)


def _patch_pointer(patch):
    buf = np.frombuffer(patch, np.uint8)
    return buf, (buf.ctypes.data_as(_u8p) if buf.size else C.cast(C.c_char_p(b"\0"), _u8p))


def patch_index(patch):
    """mpc_patch_index: validates as patch_info does -> (offset, size) of the patch's index section, (0, 0) for a version-1 patch"""
    buf, p = _patch_pointer(patch)
    at, n = C.c_size_t(0), C.c_size_t(0)
    _check(load_library().mpc_patch_index(p, buf.size, C.byref(at), C.byref(n)))
    return at.value, n.value


def patch_add_index(patch, interval=0, index_min_bytes=0):
    """mpc_patch_add_index: the patch with container_index(its container, interval) as its index section (version 2) where it has a
    container of at least max(index_min_bytes, 1) bytes whose index is not "serial only"; else the version-1 patch.  An index the patch
    carries already is dropped first."""
    L = load_library()
    buf, p = _patch_pointer(patch)
    out, nbytes = _u8p(), C.c_size_t(0)
    _check(L.mpc_patch_add_index(p, buf.size, int(interval), int(index_min_bytes), C.byref(out), C.byref(nbytes)))
    return _take_bytes(L, out, nbytes)


def patch_strip_index(patch):
    """mpc_patch_strip_index: the version-1 patch, byte for byte"""
    L = load_library()
    buf, p = _patch_pointer(patch)
    out, nbytes = _u8p(), C.c_size_t(0)
    _check(L.mpc_patch_strip_index(p, buf.size, C.byref(out), C.byref(nbytes)))
    return _take_bytes(L, out, nbytes)


def patch_info(patch):
    """mpc_patch_info: validates the patch whole -> dict(width, height, sequence, key, n, tiles, container_offset, container_bytes);
    MpcError(MPC_ERR_BITSTREAM) for a patch it refuses."""
    buf = np.frombuffer(patch, np.uint8)
    info = MpcPatchInfo()
    _check(load_library().mpc_patch_info(buf.ctypes.data_as(_u8p) if buf.size else C.cast(C.c_char_p(b"\0"), _u8p), buf.size, C.byref(info)))
    return info.as_dict()


def patch_tiles(patch):
    """mpc_patch_tiles: the patch's tile list, ascending (int32 array); a key patch's: every tile"""
    L = load_library()
    buf = np.frombuffer(patch, np.uint8)
    p = buf.ctypes.data_as(_u8p) if buf.size else C.cast(C.c_char_p(b"\0"), _u8p)
    n = C.c_int(0)
    _check(L.mpc_patch_tiles(p, buf.size, None, 0, C.byref(n)))
    tiles = np.zeros(max(n.value, 1), np.int32)
    _check(L.mpc_patch_tiles(p, buf.size, tiles.ctypes.data_as(_i32p), n.value, C.byref(n)))
    return tiles[:n.value]


class PatchDecoder:
    """mpc_patch_decoder: the receiver of a delta stream.  It keeps the current frame in device memory; apply() writes only a patch's
    listed tiles into it.  A refused patch (MpcError) leaves the frame, the list and the expected sequence as they were."""

    def __init__(self, ctx, width, height):
        self.ctx, self.L = ctx, ctx.L                               # the session must go before its context
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _check(self.L.mpc_patch_decoder_create(ctx.h, self.width, self.height, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mpc_patch_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, patch):
        """mpc_patch_apply -> patch_info's dict of the applied patch"""
        buf = np.frombuffer(patch, np.uint8)
        info = MpcPatchInfo()
        _check(self.L.mpc_patch_apply(self.h, buf.ctypes.data_as(_u8p) if buf.size else C.cast(C.c_char_p(b"\0"), _u8p), buf.size, C.byref(info)))
        return info.as_dict()

    def last_route(self):
        """mpc_patch_last_route of the last successful apply: 0 = the container's codes were parsed on the device (a version-2 patch),
        1 = serial (a version-1 patch, or the index was refused), -1 = nothing decoded (an empty patch, or no apply yet)"""
        return int(self.L.mpc_patch_last_route(self.h))

    def frame(self):
        """mpc_patch_read: the kept frame as a uint8 [H, W, 3] array"""
        out = np.empty((self.height, self.width, 3), np.uint8)
        _check(self.L.mpc_patch_read(self.h, out.ctypes.data, 0))
        return out

    def frame_device(self):
        """mpc_patch_frame_device: the kept frame's device pointer (an int): height rows of 3 * width bytes, valid until the next apply"""
        p = C.c_void_p()
        _check(self.L.mpc_patch_frame_device(self.h, C.byref(p)))
        return int(p.value or 0)

    def changed(self):
        """mpc_patch_changed: the last apply's list, ascending (int32 array); a key patch's: every tile"""
        n = C.c_int(0)
        _check(self.L.mpc_patch_changed(self.h, None, 0, C.byref(n)))
        tiles = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.mpc_patch_changed(self.h, tiles.ctypes.data_as(_i32p), n.value, C.byref(n)))
        return tiles[:n.value]


def budget_lambda(j):
    """mpc_budget_lambda: the multiplier L[j], j = 0 ... 255: 0, then (8 + (j - 1) % 8) << ((j - 1) // 8)"""
    v = C.c_uint64(0)
    _check(load_library().mpc_budget_lambda(int(j), C.byref(v)))
    return v.value


def budget_weights(index):
    """mpc_budget_weights: the rate weights W[ch, i] (uint32 [3, K], in 1/256 bit) from a seek index of a frame's full container"""
    L = load_library()
    buf = np.frombuffer(index, np.uint8)
    h = _IndexHeader()
    _check(L.mpc_index_info(buf.ctypes.data_as(_u8p), buf.size, C.byref(h)))
    weights = np.zeros((3, h.K), np.uint32)
    _check(L.mpc_budget_weights(buf.ctypes.data_as(_u8p), buf.size, weights.ctypes.data_as(_u32p)))
    return weights


def budget_allocate(profile, counts, weights, j):
    """mpc_budget_allocate: the allocation at multiplier j on the host: profile uint32 [T, K + 1], counts uint16 [T, 3], weights uint32
    [3, K] -> (depth uint8 [T], cut counts uint16 [T, 3], totals uint64 [3] = distortion, rate, records kept)"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    depth, cut, totals = np.zeros(max(T, 1), np.uint8), np.zeros((max(T, 1), 3), np.uint16), np.zeros(3, np.uint64)
    _check(load_library().mpc_budget_allocate(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p), T, K, weights.ctypes.data_as(_u32p),
                                              int(j), depth.ctypes.data_as(_u8p), cut.ctypes.data_as(_u16p),
                                              totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return depth[:T], cut[:T], totals


def owed_tiles(sent, counts, K, changed):
    """mpc_owed_tiles: sent uint8 [T], counts uint16 [T, 3], changed (ascending tile numbers) -> (candidates int32, ascending: the
    changed and the owed tiles; floor uint8 [T]; must uint8 [T]): a tile is owed iff sent[t] < max over ch of min(count, K)"""
    sent = np.ascontiguousarray(sent, np.uint8)
    T = sent.shape[0]
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    changed = np.ascontiguousarray(changed, np.int32).reshape(-1)
    cand, floor, must, n = np.zeros(max(T, 1), np.int32), np.zeros(max(T, 1), np.uint8), np.zeros(max(T, 1), np.uint8), C.c_int(0)
    _check(load_library().mpc_owed_tiles(sent.ctypes.data_as(_u8p), counts.ctypes.data_as(_u16p), T, int(K), changed.ctypes.data_as(_i32p),
                                         changed.size, cand.ctypes.data_as(_i32p), floor.ctypes.data_as(_u8p), must.ctypes.data_as(_u8p),
                                         C.byref(n)))
    return cand[:n.value], floor[:T], must[:T]


def budget_allocate_floor(profile, counts, floor, must, weights, j):
    """mpc_budget_allocate_floor: budget_allocate over candidates with a floor each (uint8 [n] or None = 0) and a must byte each (or
    None = 1) -> (depth uint8 [n], cut counts uint16 [n, 3], send uint8 [n], totals uint64 [4] = distortion, rate, records kept in the
    candidates sent, candidates sent)"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    floor = None if floor is None else np.ascontiguousarray(floor, np.uint8).reshape(T)
    must = None if must is None else np.ascontiguousarray(must, np.uint8).reshape(T)
    depth, cut, send = np.zeros(max(T, 1), np.uint8), np.zeros((max(T, 1), 3), np.uint16), np.zeros(max(T, 1), np.uint8)
    totals = np.zeros(4, np.uint64)
    _check(load_library().mpc_budget_allocate_floor(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p),
                                                    None if floor is None else floor.ctypes.data_as(_u8p),
                                                    None if must is None else must.ctypes.data_as(_u8p), T, K, weights.ctypes.data_as(_u32p),
                                                    int(j), depth.ctypes.data_as(_u8p), cut.ctypes.data_as(_u16p), send.ctypes.data_as(_u8p),
                                                    totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return depth[:T], cut[:T], send[:T], totals


class BudgetResult:
    """What encode_image_budget returns: the container (at most the budget's bytes), its seek index (None unless asked for), the depth per
    tile (uint8; K everywhere when the full container fits) and mpc_budget_info's fields."""
    __slots__ = ("container", "index", "depth", "lambda_index", "probes", "full_bytes", "sse", "full_sse", "records", "full_records")

    def __init__(self, container, index, depth, info):
        self.container, self.index, self.depth = container, index, depth
        for f, _ in MpcBudgetInfo._fields_:
            setattr(self, f, int(getattr(info, f)))

    def __repr__(self):
        return (f"BudgetResult(size={len(self.container)}, lambda_index={self.lambda_index}, probes={self.probes}, full_bytes={self.full_bytes}, "
                f"sse={self.sse}, full_sse={self.full_sse}, records={self.records}, full_records={self.full_records})")


def budget_sweep(profile, counts, weights):
    """mpc_budget_sweep: budget_allocate's totals at every multiplier on the host: profile uint32 [T, K + 1], counts uint16 [T, 3],
    weights uint32 [3, K] -> uint64 [256, 3]: distortion, rate in 1/256 bit and records kept at j = 0 ... 255"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    totals = np.zeros((MPC_BUDGET_LAMBDAS, 3), np.uint64)
    _check(load_library().mpc_budget_sweep(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p), T, K, weights.ctypes.data_as(_u32p),
                                           totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return totals


def quality_pick(totals, max_sse):
    """mpc_quality_pick: the largest multiplier j whose distortion totals[j, 0] is at most max_sse, -1 if there is none"""
    totals = np.ascontiguousarray(totals, np.uint64).reshape(MPC_BUDGET_LAMBDAS, 3)
    return int(load_library().mpc_quality_pick(totals.ctypes.data_as(C.POINTER(C.c_uint64)), int(max_sse)))


def sse_for_psnr(psnr, width, height):
    """mpc_sse_for_psnr: the largest squared error of a width x height frame whose PSNR (calculate_psnr's formula) is at least `psnr`"""
    v = C.c_uint64(0)
    _check(load_library().mpc_sse_for_psnr(float(psnr), int(width), int(height), C.byref(v)))
    return v.value


MPC_EMPHASIS_NEUTRAL, MPC_EMPHASIS_MAX = 16, 64


def _emphasis(emphasis, tiles):
    """None, or the map as uint8 [tiles]"""
    if emphasis is None:
        return None
    emphasis = np.ascontiguousarray(emphasis, np.uint8).reshape(-1)
    if emphasis.size != tiles:
        raise ValueError(f"an emphasis map of {emphasis.size} tiles for {tiles}")
    return emphasis


def _hwc_u8(rgb):
    """a host frame of the whole-frame cut encodes -> (the pixels as a contiguous uint8 [H, W, 3] array, W, H)"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("pixels: an HxWx3 uint8 array")
    return rgb, rgb.shape[1], rgb.shape[0]


def budget_allocate_emphasis(profile, counts, emphasis, weights, j):
    """mpc_budget_allocate_emphasis: budget_allocate with J = P * e[t] * 4096 + L[j] * R: emphasis uint8 [T] (16 = neutral, 0 used as 1,
    above 64 as 64) or None = neutral -> (depth, cut counts, totals); totals[0] is the unweighted squared error"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    emphasis = _emphasis(emphasis, T)
    depth, cut, totals = np.zeros(max(T, 1), np.uint8), np.zeros((max(T, 1), 3), np.uint16), np.zeros(3, np.uint64)
    _check(load_library().mpc_budget_allocate_emphasis(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p),
                                                       None if emphasis is None else emphasis.ctypes.data_as(_u8p), T, K,
                                                       weights.ctypes.data_as(_u32p), int(j), depth.ctypes.data_as(_u8p),
                                                       cut.ctypes.data_as(_u16p), totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return depth[:T], cut[:T], totals


def budget_sweep_emphasis(profile, counts, emphasis, weights):
    """mpc_budget_sweep_emphasis: budget_allocate_emphasis's totals at every multiplier -> uint64 [256, 3]"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    emphasis = _emphasis(emphasis, T)
    totals = np.zeros((MPC_BUDGET_LAMBDAS, 3), np.uint64)
    _check(load_library().mpc_budget_sweep_emphasis(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p),
                                                    None if emphasis is None else emphasis.ctypes.data_as(_u8p), T, K,
                                                    weights.ctypes.data_as(_u32p), totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return totals


def budget_allocate_floor_emphasis(profile, counts, floor, must, emphasis, tile_list, weights, j):
    """mpc_budget_allocate_floor_emphasis: budget_allocate_floor with an emphasis map of the whole frame (uint8 [tiles] or None);
    candidate i takes emphasis[tile_list[i]] (int32 [n]; None = the identity), the neutral value where that is outside the frame
    -> (depth, cut counts, send, totals uint64 [4]); totals[0] is unweighted"""
    profile = np.ascontiguousarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(3, K)
    floor = None if floor is None else np.ascontiguousarray(floor, np.uint8).reshape(T)
    must = None if must is None else np.ascontiguousarray(must, np.uint8).reshape(T)
    emphasis = None if emphasis is None else np.ascontiguousarray(emphasis, np.uint8).reshape(-1)
    tile_list = None if tile_list is None else np.ascontiguousarray(tile_list, np.int32).reshape(T)
    depth, cut, send = np.zeros(max(T, 1), np.uint8), np.zeros((max(T, 1), 3), np.uint16), np.zeros(max(T, 1), np.uint8)
    totals = np.zeros(4, np.uint64)
    _check(load_library().mpc_budget_allocate_floor_emphasis(
        profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p), None if floor is None else floor.ctypes.data_as(_u8p),
        None if must is None else must.ctypes.data_as(_u8p), None if emphasis is None else emphasis.ctypes.data_as(_u8p),
        None if tile_list is None else tile_list.ctypes.data_as(_i32p), 0 if emphasis is None else emphasis.size, T, K,
        weights.ctypes.data_as(_u32p), int(j), depth.ctypes.data_as(_u8p), cut.ctypes.data_as(_u16p), send.ctypes.data_as(_u8p),
        totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return depth[:T], cut[:T], send[:T], totals


def emphasis_from_mask(mask, lo=1, hi=MPC_EMPHASIS_MAX, width=None):
    """mpc_emphasis_from_mask: a uint8 mask at pixel resolution, [H, W] with any row stride and alignment (a numpy view is read in place
    when its last axis is contiguous; width: the frame's, where the rows are wider than it) -> emphasis uint8 [tiles], t = tx * tiles_y
    + ty: lo + ((hi - lo) * m + 127) // 255, m the largest mask byte of the tile's pixels inside the frame"""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.ndim != 2:
        raise ValueError("the mask: an HxW uint8 array")
    if mask.shape[1] > 1 and mask.strides[1] != 1 or mask.shape[0] > 1 and mask.strides[0] < mask.shape[1]:
        mask = np.ascontiguousarray(mask)
    H, W = mask.shape[0], mask.shape[1] if width is None else int(width)
    stride = mask.strides[0] if H > 1 else max(W, 1)
    tiles = -(-max(W, 0) // 8) * -(-H // 8)
    out = np.zeros(max(tiles, 1), np.uint8)
    _check(load_library().mpc_emphasis_from_mask(C.c_void_p(mask.ctypes.data), W, H, stride, int(lo), int(hi), out.ctypes.data_as(_u8p)))
    return out[:tiles]


class QualityResult:
    """What encode_image_quality returns: the container, its seek index (None unless asked for), the depth per tile (uint8) and
    mpc_quality_info's fields; sse is at most the target."""
    __slots__ = ("container", "index", "depth", "lambda_index", "full_bytes", "sse", "full_sse", "min_sse", "records", "full_records",
                 "model_bits_256")

    def __init__(self, container, index, depth, info):
        self.container, self.index, self.depth = container, index, depth
        for f, _ in MpcQualityInfo._fields_:
            setattr(self, f, int(getattr(info, f)))

    def __repr__(self):
        return (f"QualityResult(size={len(self.container)}, lambda_index={self.lambda_index}, full_bytes={self.full_bytes}, sse={self.sse}, "
                f"full_sse={self.full_sse}, min_sse={self.min_sse}, records={self.records}, full_records={self.full_records}, "
                f"model_bits_256={self.model_bits_256})")


MPC_GROUP_MAX_FRAMES = 64


def _group_arrays(profile, counts, emphasis, weights):
    """a group's arrays as the library takes them: profile uint32 [F, T, K + 1], counts uint16 [F, T, 3], emphasis None or uint8 [F, T],
    weights uint32 [F, 3, K] -> (profile, counts, emphasis, weights, F, T, K)"""
    profile = np.ascontiguousarray(profile, np.uint32)
    if profile.ndim != 3:
        raise ValueError("a group's profile: [frames, tiles, K + 1]")
    F, T, K = profile.shape[0], profile.shape[1], profile.shape[2] - 1
    counts = np.ascontiguousarray(counts, np.uint16).reshape(F, T, 3)
    weights = np.ascontiguousarray(weights, np.uint32).reshape(F, 3, K)
    return profile, counts, _emphasis(emphasis, F * T), weights, F, T, K


def budget_allocate_group(profile, counts, emphasis, weights, j):
    """mpc_budget_allocate_group: the allocation at multiplier j over a group of frames, every frame with its own weights: profile uint32
    [F, T, K + 1], counts uint16 [F, T, 3], emphasis uint8 [F, T] or None, weights uint32 [F, 3, K] -> (depth uint8 [F, T], cut counts
    uint16 [F, T, 3], totals uint64 [F, 3])"""
    profile, counts, emphasis, weights, F, T, K = _group_arrays(profile, counts, emphasis, weights)
    depth, cut, totals = np.zeros((F, max(T, 1)), np.uint8), np.zeros((F, max(T, 1), 3), np.uint16), np.zeros((max(F, 1), 3), np.uint64)
    if T == 0:
        depth, cut = depth[:, :0], cut[:, :0]
    _check(load_library().mpc_budget_allocate_group(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p),
                                                    None if emphasis is None else emphasis.ctypes.data_as(_u8p), F, T, K,
                                                    weights.ctypes.data_as(_u32p), int(j), depth.ctypes.data_as(_u8p) if T else None,
                                                    cut.ctypes.data_as(_u16p) if T else None, totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return depth, cut, totals[:F]


def budget_sweep_group(profile, counts, emphasis, weights):
    """mpc_budget_sweep_group: the group allocation's totals, summed over the frames, at every multiplier -> uint64 [256, 3]"""
    profile, counts, emphasis, weights, F, T, K = _group_arrays(profile, counts, emphasis, weights)
    totals = np.zeros((MPC_BUDGET_LAMBDAS, 3), np.uint64)
    _check(load_library().mpc_budget_sweep_group(profile.ctypes.data_as(_u32p), counts.ctypes.data_as(_u16p),
                                                 None if emphasis is None else emphasis.ctypes.data_as(_u8p), F, T, K,
                                                 weights.ctypes.data_as(_u32p), totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return totals


def sse_for_psnr_group(psnr, width, height, frames):
    """mpc_sse_for_psnr_group: the largest squared error of `frames` width x height frames together whose PSNR over all their pixels
    (calculate_psnr's formula) is at least `psnr`; frames = 1: sse_for_psnr"""
    v = C.c_uint64(0)
    _check(load_library().mpc_sse_for_psnr_group(float(psnr), int(width), int(height), int(frames), C.byref(v)))
    return v.value


class GroupResult:
    """What encode_images_budget and encode_images_quality return: `frames`, a list of BudgetResult or QualityResult, one per frame in
    order (len(), indexing and iteration go to it), and `info`, the same info fields summed over the group (lambda_index and probes
    once), a BudgetResult or QualityResult without container, index and depth."""
    __slots__ = ("frames", "info")

    def __init__(self, frames, info):
        self.frames, self.info = frames, info

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]

    def __iter__(self):
        return iter(self.frames)

    @property
    def size(self):
        """the containers' bytes together"""
        return sum(len(f.container) for f in self.frames)

    def __repr__(self):
        return f"GroupResult(frames={len(self.frames)}, size={self.size}, info={self.info!r})"


def _view_parse(fn, head, buf, idx, view, parse_all):
    _, _, K, _ = container_info(buf)
    vw = _view(view)
    ranges = np.zeros((3 * K, 2), np.uint64)
    out, n, route = _u16p(), C.c_size_t(0), C.c_int(-1)
    _check(fn(*head, buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size, C.byref(vw), 1 if parse_all else 0, C.byref(out),
              C.byref(n), ranges.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(route)))
    return _take_u16(load_library(), out, n), ranges, route.value


def parse_container_view_by_index(blob, index, view, parse_all=False):
    """mpc_parse_container_view_by_index: the host definition of a view's device parse, view = (rect, steps, scale_log2) ->
    (symbols, ranges, route) as parse_container_window_by_index gives them for truncate_container(blob, steps): the lengths cut to
    `steps`, the streams of steps at or above it empty."""
    buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
    return _view_parse(load_library().mpc_parse_container_view_by_index, (), buf, idx, view, parse_all)


def parse_container_by_index(blob, index):
    """mpc_parse_container_by_index: the chunked parse on the host -> (symbols, route): the lengths stream and the 6K coded
    streams of read_compressed(coded=True) back to back (uint16); route 0 = the index was used, 1 = refused, the serial parse's
    result.  MpcError as read_compressed(coded=True) raises it."""
    L = load_library()
    buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
    out, n, route = _u16p(), C.c_size_t(0), C.c_int(-1)
    _check(L.mpc_parse_container_by_index(buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size, C.byref(out),
                                          C.byref(n), C.byref(route)))
    return _take_u16(L, out, n), route.value


def decode_image(blob, ctx):
    """compressed::decodeImage (CompressedImage.h:75) -> uint8 [H,W,3]; reconstructed on ctx's device (no host path)."""
    L = load_library()
    buf = np.frombuffer(blob, np.uint8)                      # no copy of the container: bytes, bytearray and arrays alike
    out, W, H = _u8p(), C.c_int(), C.c_int()
    _check(L.mpc_decode_image(ctx.h, buf.ctypes.data_as(_u8p), buf.size, C.byref(out),
                              C.byref(W), C.byref(H)))
    # the pixels stay in the buffer the library returned (the array owns it and frees it with mpc_free): no 48 MB copy per frame
    img = _take_view(L, out, C.c_size_t(3 * W.value * H.value)).reshape(H.value, W.value, 3)
    return img


def calculate_psnr(original, decoded):
    """compressed::calculatePSNR (CompressedImage.h:57)."""
    L = load_library()
    a = np.ascontiguousarray(original, np.uint8)
    b = np.ascontiguousarray(decoded, np.uint8)
    return L.mpc_psnr(a.ctypes.data_as(_u8p), b.ctypes.data_as(_u8p), a.shape[1], a.shape[0])


def quant_tables(K, bpp, block_size=8):
    """createQuantizationTables (CompressedImage.cpp:124-166) without a context -> float64 [3, K] (Y, U, V)."""
    L = load_library()
    q = np.zeros((3, int(K)), np.float64)
    _check(L.mpc_quant_tables(int(K), int(block_size), float(bpp), q.ctypes.data_as(_dp)))
    return q


def parse_qualities(qualities, K, block_size=8):
    """The levels of a rate-distortion sweep -> (labels, quants float64 [n, 3, K]).  An item is a bpp allocation (a number:
    createQuantizationTables' table), "max" (every step 1.0, Compression.cpp:104-110) or an explicit [3, K] table (label
    "table").  A single item may be given without a list."""
    if isinstance(qualities, (str, bytes, int, float, np.floating, np.integer)) or (
            isinstance(qualities, np.ndarray) and qualities.ndim == 2):
        qualities = [qualities]
    labels, tables = [], []
    for q in qualities:
        if isinstance(q, str):
            if q != "max":
                raise ValueError(f"quality {q!r}: a bpp allocation, 'max' or a [3, {K}] table")
            labels.append("max")
            tables.append(np.ones((3, K)))
        elif isinstance(q, (int, float, np.floating, np.integer)) and not isinstance(q, bool):
            if not np.isfinite(q):
                raise ValueError(f"quality {q!r}: bpp allocation must be finite")
            labels.append(float(q))
            tables.append(quant_tables(K, float(q), block_size))
        else:
            a = np.asarray(q, np.float64)
            if a.shape != (3, K):
                raise ValueError(f"quality table of shape {a.shape}, expected (3, {K})")
            labels.append("table")
            tables.append(a)
    if not tables:
        raise ValueError("no quality levels")
    return labels, np.ascontiguousarray(np.stack(tables), np.float64)


class RatePoint:
    """One level of a rate-distortion sweep (Compression.cpp -g's row): quality label, container size in bytes, bpp =
    8 * size / (width * height) as Compression.cpp:177 computes it, the exact squared error, calculatePSNR's value and
    (keep_bytes) the container."""
    __slots__ = ("quality", "quant", "size", "bpp", "sse", "psnr", "container")

    def __init__(self, quality, quant, size, bpp, sse, psnr, container):
        self.quality, self.quant, self.size, self.bpp, self.sse, self.psnr, self.container = (
            quality, quant, size, bpp, sse, psnr, container)

    def __repr__(self):
        return f"RatePoint(quality={self.quality!r}, size={self.size}, bpp={self.bpp!r}, sse={self.sse}, psnr={self.psnr!r})"


def format_double(v):
    """std::format("{}", double) as the reference's reports print numbers (shortest round-trip text)."""
    buf = C.create_string_buffer(64)
    n = load_library().mpc_format_double(float(v), buf, 64)
    if n < 0:
        raise ValueError("buffer too small")
    return buf.value.decode()


class PatchStatistics:
    """The "-s" mode of Compression.cpp:200-302: random patches of every image through CalcMPDynamic with all
    quantisers 1.0 (on ctx's device), Welford statistics of intCoeff / deltaId per step, and the text report."""

    def __init__(self, ctx, seed):
        self.L = load_library()
        self.ctx = ctx
        self.h = None
        h = C.c_void_p()
        _check(self.L.mpc_patch_stats_create(ctx.h, int(seed), C.byref(h)))
        self.h = h

    def add_image(self, rgb, patches):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        H, W, _ = rgb.shape
        _check(self.L.mpc_patch_stats_add_image(self.h, rgb.ctypes.data_as(_u8p), W, H, int(patches)))

    def read(self):
        """[3 channels][intCoeff, deltaId][K steps][N, min, max, mean, sumSq]"""
        out = np.zeros((3, 2, self.ctx.K, 5), np.float64)
        _check(self.L.mpc_patch_stats_read(self.h, out.ctypes.data_as(_dp)))
        return out

    def report(self):
        text, n = C.c_char_p(), C.c_size_t()
        _check(self.L.mpc_patch_stats_report(self.h, C.byref(text), C.byref(n)))
        out = C.string_at(text, n.value).decode()
        self.L.mpc_free(C.cast(text, C.c_void_p))
        return out

    def close(self):
        if self.h:
            self.L.mpc_patch_stats_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _check(st):
    if st != MPC_OK:
        raise MpcError(st, load_library().mpc_last_error().decode())


CHOICE_DTYPE = np.dtype([("deltaId", "<u2"), ("intCoeff", "<u2")])


class CompressionContext:
    """compressed::CompressionContext (CompressedImage.h:28-36): K, BlockSize, the dictionary and the three
    quantisation tables; `device` >= 0 uploads the dictionary once to that GPU."""

    def __init__(self, K=32, block_size=8, bpp=3.5, device=-1):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.mpc_context_create(int(K), int(block_size), float(bpp), int(device), C.byref(h)))
        self.h = h
        self.K = K
        self.block_size = block_size
        self.device = device
        self.num_base = self.L.mpc_context_num_base(h)
        self.detail_rows = self.L.mpc_context_detail_rows(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.mpc_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- tables ----------------------------------------------------------------------------------
    def set_fast(self, on=True):
        """mpc_context_set_fast: the `...Fast` (float) flavour of the tile path for every later encode / decode of this context."""
        _check(self.L.mpc_context_set_fast(self.h, 1 if on else 0))
        return self

    @property
    def fast(self):
        return bool(self.L.mpc_context_is_fast(self.h))

    @property
    def quant(self):
        q = np.zeros((3, self.K), np.float64)
        _check(self.L.mpc_context_get_quant(self.h, q.ctypes.data_as(_dp)))
        return q

    def set_quant(self, q):
        q = np.ascontiguousarray(q, np.float64).reshape(3, self.K)
        _check(self.L.mpc_context_set_quant(self.h, q.ctypes.data_as(_dp)))

    def dictionary(self):
        """-> base[num_base,64], block_rows[num_base], detail[3][detail_rows,64] (host copies)."""
        n = self.block_size * self.block_size
        base = np.zeros((self.num_base, n))
        rows = np.zeros(self.num_base, np.int32)
        det = [np.zeros((self.detail_rows, n)) for _ in range(3)]
        _check(self.L.mpc_context_get_dictionary(self.h, base.ctypes.data_as(_dp), rows.ctypes.data_as(_i32p),
                                                 det[0].ctypes.data_as(_dp), det[1].ctypes.data_as(_dp),
                                                 det[2].ctypes.data_as(_dp)))
        return base, rows, det

    def set_tile_encode_workgroups(self, workgroups):
        """mpc_context_set_tile_encode_workgroups: CUs the tile encode may fill (0 = all), for callers with other work on the device."""
        _check(self.L.mpc_context_set_tile_encode_workgroups(self.h, int(workgroups)))

    @property
    def max_waves(self):
        return self.L.mpc_context_max_waves(self.h)

    # -- hot path --------------------------------------------------------------------------------
    def encode_tiles(self, rgb, tile_row_begin=0, tile_row_end=None, quant=None):
        """Host-buffer form. rgb: uint8 [H,W,3]. Returns counts[T,3], choices[T,3,K] (structured),
        energy[T,3], swept[T,3]; tile t = tx*rows + (ty - tile_row_begin).
        A view whose pixels are contiguous within a row (strides[1:] == (3, 1), e.g. a window of a larger image) is passed as
        it is, strides[0] as row_stride, without a copy; anything else is made contiguous first."""
        rgb = np.asarray(rgb)
        if not (rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.strides[1:] == (3, 1)
                and rgb.strides[0] >= 3 * rgb.shape[1]):
            rgb = np.ascontiguousarray(rgb, np.uint8)
        H, W = rgb.shape[:2]
        row_stride = rgb.strides[0]
        ty = (H + 7) // 8
        tx = (W + 7) // 8
        tile_row_end = ty if tile_row_end is None else tile_row_end
        T = tx * (tile_row_end - tile_row_begin)
        counts = np.zeros((T, 3), np.uint16)
        choices = np.zeros((T, 3, self.K), CHOICE_DTYPE)
        energy = np.zeros((T, 3), np.float64)
        swept = np.zeros((T, 3), np.uint32)
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_encode_tiles(self.h, rgb.ctypes.data_as(_u8p), W, H, row_stride, tile_row_begin, tile_row_end, qp,
                                       counts.ctypes.data_as(_u16p), choices.ctypes.data_as(C.c_void_p),
                                       energy.ctypes.data_as(_dp), swept.ctypes.data_as(_u32p)))
        return counts, choices, energy, swept

    def encode_tiles_device(self, d_rgb, width, height, row_stride, tile_row_begin, tile_row_end,
                            d_counts, d_choices, d_energy=0, d_swept=0, quant=None, waves=0, stream=0):
        """Device-pointer form (ints from tensor.data_ptr()); asynchronous on `stream` (hipStream_t int)."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_encode_tiles_device(self.h, d_rgb, width, height, row_stride, tile_row_begin, tile_row_end,
                                              qp, d_counts, d_choices, d_energy or None, d_swept or None,
                                              waves, stream or None))

    def encode_batch_device(self, d_rgb, frames, frame_stride, width, height, row_stride, tile_row_begin, tile_row_end,
                            d_counts, d_choices, d_energy=0, d_swept=0, quant=None, waves=0, stream=0):
        """`frames` frames `frame_stride` bytes apart, same tile rows of each, one launch."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_encode_batch_device(self.h, d_rgb, frames, frame_stride, width, height, row_stride,
                                              tile_row_begin, tile_row_end, qp, d_counts, d_choices,
                                              d_energy or None, d_swept or None, waves, stream or None))

    def histogram_device(self, d_counts, d_choices, tiles, d_hist, stream=0):
        _check(self.L.mpc_histogram_device(self.h, d_counts, d_choices, tiles, d_hist, stream or None))

    def reserve(self, max_tiles):
        """Pre-allocate the device workspace for calls of up to `max_tiles` tiles."""
        _check(self.L.mpc_reserve(self.h, int(max_tiles)))

    def kernel_timing(self, on=True):
        """Bracket every base-sweep launch with HIP events on the launch stream (measurement only)."""
        self.L.mpc_kernel_timing_enable(self.h, 1 if on else 0)

    def read_kernel_timing(self):
        """-> (summed base-sweep ms, launches, ms of the union of the launch intervals) since the last read."""
        ms, n, busy = C.c_double(0), C.c_longlong(0), C.c_double(0)
        _check(self.L.mpc_kernel_timing_read(self.h, C.byref(ms), C.byref(n), C.byref(busy)))
        return ms.value, n.value, busy.value

    def read_kernel_counters(self):
        """-> (MFMA instructions executed, tile-channel-steps) counted by the pursuit kernel since kernel_timing(True) / the last read."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        _check(self.L.mpc_kernel_counters_read(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def encode_image(self, rgb, quant=None, view=False):
        """compressed::encodeImage (CompressedImage.h:59) -> bytes (view=True: a read-only uint8 array on the buffer the library
        returned, as a C caller holds it: no Python-side copy of the container)."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        H, W = rgb.shape[:2]
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        out, n = _u8p(), C.c_size_t(0)
        _check(self.L.mpc_encode_image(self.h, rgb.ctypes.data_as(_u8p), W, H, qp, C.byref(out), C.byref(n)))
        return (_take_view if view else _take_bytes)(self.L, out, n)

    def encode_images(self, frames, quant=None, views=False):
        """encodeImage for a sequence of equally sized frames in host memory, pipelined (mpc_encode_images).  Returns a list of
        bytes objects; views=True: read-only uint8 arrays on the library's buffers (no Python-side copy)."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        H, W = frames[0].shape[:2]
        if any(f.shape[:2] != (H, W) for f in frames):
            raise ValueError("frames must have the same size")
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        n = len(frames)
        ptrs = (_u8p * n)(*[f.ctypes.data_as(_u8p) for f in frames])
        outs = (_u8p * n)()
        sizes = (C.c_size_t * n)()
        _check(self.L.mpc_encode_images(self.h, ptrs, n, W, H, qp, outs, sizes))
        take = _take_view if views else _take_bytes
        return [take(self.L, outs[i], C.c_size_t(sizes[i])) for i in range(n)]

    def encode_images_device(self, d_frames, width, height, quant=None, views=False):
        """mpc_encode_images_device: frames already in device memory (ints from tensor.data_ptr(), tightly packed RGB).
        Returns a list of bytes objects (containers), pipelined like encode_images; views=True: read-only uint8 arrays on the
        buffers the library returned instead (what a C caller holds: no Python-side copy of every container)."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        n = len(d_frames)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in d_frames])
        outs = (_u8p * n)()
        sizes = (C.c_size_t * n)()
        _check(self.L.mpc_encode_images_device(self.h, ptrs, n, width, height, qp, outs, sizes))
        take = _take_view if views else _take_bytes
        return [take(self.L, outs[i], C.c_size_t(sizes[i])) for i in range(n)]

    def _indexed(self, fn, ptrs, n, width, height, interval, quant, flags=None):
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        outs, sizes, idx, isizes = (_u8p * n)(), (C.c_size_t * n)(), (_u8p * n)(), (C.c_size_t * n)()
        if flags is None:
            _check(fn(self.h, ptrs, n, width, height, qp, int(interval), outs, sizes, idx, isizes))
        else:                                                       # the ...indexed2 entry points
            _check(fn(self.h, ptrs, n, width, height, qp, int(interval), int(flags), outs, sizes, idx, isizes))
        return [(_take_bytes(self.L, outs[i], C.c_size_t(sizes[i])), _take_bytes(self.L, idx[i], C.c_size_t(isizes[i]))) for i in range(n)]

    def encode_images_indexed(self, frames, interval=0, quant=None, expanded=False):
        """mpc_encode_images_indexed: encode_images with every container's seek index from the entropy stage itself ->
        [(container, index)], index == container_index(container, interval).  interval: 0 = the default, else 32 ... 65536.
        expanded: index version 2 (mpc_encode_images_indexed2 with MPC_INDEX_EXPANDED), the aux entries from the entropy stage as
        well: index == container_index(container, interval, expanded=True)."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        H, W = frames[0].shape[:2]
        if any(f.shape[:2] != (H, W) for f in frames):
            raise ValueError("frames must have the same size")
        n = len(frames)
        ptrs = (_u8p * n)(*[f.ctypes.data_as(_u8p) for f in frames])
        if expanded:
            return self._indexed(self.L.mpc_encode_images_indexed2, ptrs, n, W, H, interval, quant, MPC_INDEX_EXPANDED)
        return self._indexed(self.L.mpc_encode_images_indexed, ptrs, n, W, H, interval, quant)

    def encode_images_indexed_device(self, d_frames, width, height, interval=0, quant=None, expanded=False):
        """mpc_encode_images_indexed_device: the same for frames in device memory (as encode_images_device takes them)."""
        n = len(d_frames)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in d_frames])
        if expanded:
            return self._indexed(self.L.mpc_encode_images_indexed2_device, ptrs, n, width, height, interval, quant, MPC_INDEX_EXPANDED)
        return self._indexed(self.L.mpc_encode_images_indexed_device, ptrs, n, width, height, interval, quant)

    def encode_image_device(self, d_rgb, width, height, quant=None):
        return self.encode_images_device([d_rgb], width, height, quant)[0]

    # -- sequence decode ---------------------------------------------------------------------------
    @staticmethod
    def _containers(blobs):
        bufs = [np.frombuffer(b, np.uint8) for b in blobs]       # no copy: bytes, bytearray and arrays alike
        n = len(bufs)
        return bufs, (_u8p * n)(*[b.ctypes.data_as(_u8p) for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs])

    def decode_images(self, blobs):
        """mpc_decode_images: decodeImage for a list of containers in one call (parsed side by side, pipelined on the device).
        Returns a list of uint8 [H,W,3] arrays on the library's buffers, as decode_image returns them."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        outs, W, H = (_u8p * n)(), (C.c_int * n)(), (C.c_int * n)()
        _check(self.L.mpc_decode_images(self.h, ptrs, sizes, n, outs, W, H))
        return [_take_view(self.L, outs[i], C.c_size_t(3 * W[i] * H[i])).reshape(H[i], W[i], 3) for i in range(n)]

    def decode_images_device(self, blobs, out=None):
        """mpc_decode_images_device: the same with the pixels left on the context's device.  out: a list of contiguous uint8
        torch tensors there, each of at least 3*W*H elements (bytes behind that are left alone); None = allocated here from
        container_info.  Returns a list of uint8 [H,W,3] tensors (views of `out` where given)."""
        import torch
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        if out is None:
            out = []
            for b in bufs:
                try:
                    w, h, _, _ = container_info(b)
                except MpcError:                                 # the call itself refuses the frame, in its turn, by its index
                    w, h = 1, 1
                out.append(torch.empty(3 * w * h, dtype=torch.uint8, device=f"cuda:{self.device}"))
        if len(out) != n or any(t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() for t in out):
            raise ValueError("out: one contiguous uint8 device tensor per container")
        d_ptrs = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in out])
        caps = (C.c_size_t * n)(*[t.numel() for t in out])
        W, H = (C.c_int * n)(), (C.c_int * n)()
        torch.cuda.synchronize(self.device)                      # `out` may still be being written by the caller's streams
        _check(self.L.mpc_decode_images_device(self.h, ptrs, sizes, n, d_ptrs, caps, W, H))
        return [out[i].view(-1)[:3 * W[i] * H[i]].view(H[i], W[i], 3) for i in range(n)]

    def decode_image_device(self, blob, out=None):
        return self.decode_images_device([blob], None if out is None else [out])[0]

    @staticmethod
    def _indexes(indexes, n):
        if len(indexes) != n:
            raise ValueError("one index (or None) per container")
        bufs = [None if x is None else np.frombuffer(x, np.uint8) for x in indexes]
        ptrs = (_u8p * n)(*[_u8p() if b is None else b.ctypes.data_as(_u8p) for b in bufs])
        return bufs, ptrs, (C.c_size_t * n)(*[0 if b is None else b.size for b in bufs])

    def decode_images_indexed(self, blobs, indexes):
        """mpc_decode_images_indexed: decode_images with a seek index (container_index) per container, None = without: a frame
        with an index has its entropy codes parsed on the device.  Returns (frames, routes), routes[f] 0 = parsed on the device,
        1 = the serial route.  Pixels and errors are decode_images's, whatever an index holds."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        outs, W, H, routes = (_u8p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        _check(self.L.mpc_decode_images_indexed(self.h, ptrs, sizes, iptrs, isizes, n, outs, W, H, routes))
        return [_take_view(self.L, outs[i], C.c_size_t(3 * W[i] * H[i])).reshape(H[i], W[i], 3) for i in range(n)], list(routes)

    def decode_images_indexed_device(self, blobs, indexes, out=None):
        """mpc_decode_images_indexed_device: the same with the pixels left on the context's device (`out` as for
        decode_images_device).  Returns (frames, routes)."""
        import torch
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        if out is None:
            out = []
            for b in bufs:
                try:
                    w, h, _, _ = container_info(b)
                except MpcError:                                 # the call itself refuses the frame, in its turn, by its index
                    w, h = 1, 1
                out.append(torch.empty(3 * w * h, dtype=torch.uint8, device=f"cuda:{self.device}"))
        if len(out) != n or any(t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() for t in out):
            raise ValueError("out: one contiguous uint8 device tensor per container")
        d_ptrs = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in out])
        caps = (C.c_size_t * n)(*[t.numel() for t in out])
        W, H, routes = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        torch.cuda.synchronize(self.device)                      # `out` may still be being written by the caller's streams
        _check(self.L.mpc_decode_images_indexed_device(self.h, ptrs, sizes, iptrs, isizes, n, d_ptrs, caps, W, H, routes))
        return [out[i].view(-1)[:3 * W[i] * H[i]].view(H[i], W[i], 3) for i in range(n)], list(routes)

    def container_index_device(self, blob, interval=0, flags=0):
        """mpc_container_index_device: container_index2's blob with the checkpoints found by the device's bit scan instead of a
        serial parse -> (index, route).  route 0 = the scan produced the blob and the device parse accepted it, 1 = the host
        builder ran.  Status, text and blob are container_index2's for every input."""
        buf = np.frombuffer(blob, np.uint8)
        out, n, route = _u8p(), C.c_size_t(0), C.c_int(-1)
        _check(self.L.mpc_container_index_device(self.h, buf.ctypes.data_as(_u8p), buf.size, int(interval), int(flags), C.byref(out), C.byref(n),
                                                 C.byref(route)))
        return _take_bytes(self.L, out, n), route.value

    def debug_container_index_device(self, blob, interval=0, segment_bits=0, window_bits=0):
        """mpc_debug_container_index_device: container_index_device (flags 0) with the scan's segment and window sizes given, so
        that a test can make a chain cross windows and a code jump segments on a small container -> (index, route)"""
        buf = np.frombuffer(blob, np.uint8)
        out, n, route = _u8p(), C.c_size_t(0), C.c_int(-1)
        _check(self.L.mpc_debug_container_index_device(self.h, buf.ctypes.data_as(_u8p), buf.size, int(interval), int(segment_bits),
                                                       int(window_bits), C.byref(out), C.byref(n), C.byref(route)))
        return _take_bytes(self.L, out, n), route.value

    def _scanned_indexes(self, n, routes, idx, idx_n):
        return [_take_bytes(self.L, idx[i], C.c_size_t(idx_n[i])) if routes[i] == 0 and idx[i] else None for i in range(n)]

    def decode_images_scan(self, blobs, keep_indexes=False):
        """mpc_decode_images_scan: decode_images for containers that come without a seek index: per frame one upload, the device's
        bit scan for the checkpoints, then the indexed route on the bytes already on the device.  Returns (frames, routes),
        routes[f] 0 = scanned and parsed on the device, 1 = the serial route; with keep_indexes (frames, routes, indexes), indexes[f]
        the version-1 index of a frame on route 0 (== container_index(blob)), None on route 1.  Pixels and errors are decode_images's."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        outs, W, H, routes = (_u8p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        idx, idx_n = ((_u8p * n)(), (C.c_size_t * n)()) if keep_indexes else (None, None)
        _check(self.L.mpc_decode_images_scan(self.h, ptrs, sizes, n, outs, W, H, idx, idx_n, routes))
        frames = [_take_view(self.L, outs[i], C.c_size_t(3 * W[i] * H[i])).reshape(H[i], W[i], 3) for i in range(n)]
        if not keep_indexes:
            return frames, list(routes)
        return frames, list(routes), self._scanned_indexes(n, routes, idx, idx_n)

    def decode_images_scan_device(self, blobs, out=None, keep_indexes=False):
        """mpc_decode_images_scan_device: the same with the pixels left on the context's device (`out` as for
        decode_images_device).  Returns (frames, routes), or (frames, routes, indexes) with keep_indexes."""
        import torch
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        if out is None:
            out = []
            for b in bufs:
                try:
                    w, h, _, _ = container_info(b)
                except MpcError:                                 # the call itself refuses the frame, in its turn
                    w, h = 1, 1
                out.append(torch.empty(3 * w * h, dtype=torch.uint8, device=f"cuda:{self.device}"))
        if len(out) != n or any(t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() for t in out):
            raise ValueError("out: one contiguous uint8 device tensor per container")
        d_ptrs = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in out])
        caps = (C.c_size_t * n)(*[t.numel() for t in out])
        W, H, routes = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        idx, idx_n = ((_u8p * n)(), (C.c_size_t * n)()) if keep_indexes else (None, None)
        torch.cuda.synchronize(self.device)                      # `out` may still be being written by the caller's streams
        _check(self.L.mpc_decode_images_scan_device(self.h, ptrs, sizes, n, d_ptrs, caps, W, H, idx, idx_n, routes))
        frames = [out[i].view(-1)[:3 * W[i] * H[i]].view(H[i], W[i], 3) for i in range(n)]
        if not keep_indexes:
            return frames, list(routes)
        return frames, list(routes), self._scanned_indexes(n, routes, idx, idx_n)

    @staticmethod
    def _rects(rects, n):
        if len(rects) != n:
            raise ValueError("one rectangle (x, y, width, height) per container")
        return (MpcRect * n)(*[MpcRect(*[int(v) for v in r]) for r in rects])

    def decode_regions(self, blobs, indexes, rects, parse_all=False):
        """mpc_decode_regions_indexed: the pixel rectangle rects[f] = (x, y, width, height) of every frame, through the frame's
        seek index (None = without) -> (frames, routes): uint8 [height, width, 3] arrays, routes[f] 0 = only the rectangle's window
        of the streams was parsed and reconstructed, 1 = the whole frame by the serial route, cropped.  parse_all: every chunk of
        every stream is parsed (MPC_REGION_PARSE_ALL: the index is then a hint only, as for a whole frame)."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        rc = self._rects(rects, n)
        outs, routes = (_u8p * n)(), (C.c_int * n)()
        _check(self.L.mpc_decode_regions_indexed(self.h, ptrs, sizes, iptrs, isizes, rc, n, 1 if parse_all else 0, outs, routes))
        return [_take_view(self.L, outs[i], C.c_size_t(3 * rc[i].width * rc[i].height)).reshape(rc[i].height, rc[i].width, 3)
                for i in range(n)], list(routes)

    def decode_regions_device(self, blobs, indexes, rects, parse_all=False, out=None):
        """mpc_decode_regions_indexed_device: the same with the pixels left on the context's device.  out: a list of contiguous
        uint8 torch tensors there, each of at least 3 * width * height elements of its rectangle (bytes behind that are left
        alone); None = allocated here.  Returns (frames, routes), the frames uint8 [height, width, 3] tensors."""
        import torch
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        rc = self._rects(rects, n)
        if out is None:
            out = [torch.empty(3 * max(r.width, 1) * max(r.height, 1), dtype=torch.uint8, device=f"cuda:{self.device}") for r in rc]
        if len(out) != n or any(t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() for t in out):
            raise ValueError("out: one contiguous uint8 device tensor per container")
        d_ptrs = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in out])
        caps = (C.c_size_t * n)(*[t.numel() for t in out])
        routes = (C.c_int * n)()
        torch.cuda.synchronize(self.device)                      # `out` may still be being written by the caller's streams
        _check(self.L.mpc_decode_regions_indexed_device(self.h, ptrs, sizes, iptrs, isizes, rc, n, 1 if parse_all else 0, d_ptrs, caps,
                                                        routes))
        return [out[i].view(-1)[:3 * rc[i].width * rc[i].height].view(rc[i].height, rc[i].width, 3) for i in range(n)], list(routes)

    @staticmethod
    def _views(views, n):
        if len(views) != n:
            raise ValueError("one view (rect, steps, scale_log2) per container")
        return (MpcView * n)(*[_view(v) for v in views])

    def decode_views(self, blobs, indexes, views, parse_all=False):
        """mpc_decode_views_indexed: views[f] = (rect, steps, scale_log2) of every frame -- the rectangle (x, y, width, height),
        None = the whole frame, reconstructed from the first `steps` records of every tile-channel (0 = all) and reduced by
        2^scale_log2 (0 ... 3; the rectangle's origin a multiple of it) -> (frames, routes): uint8 [ceil(height / c), ceil(width / c), 3]
        arrays, routes[f] 0 = through the frame's seek index, the streams of steps at or above `steps` never read, 1 = the serial
        parse.  parse_all: MPC_VIEW_PARSE_ALL."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        vw = self._views(views, n)
        outs, W, H, routes = (_u8p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        _check(self.L.mpc_decode_views_indexed(self.h, ptrs, sizes, iptrs, isizes, vw, n, 1 if parse_all else 0, outs, W, H, routes))
        return [_take_view(self.L, outs[i], C.c_size_t(3 * W[i] * H[i])).reshape(H[i], W[i], 3) for i in range(n)], list(routes)

    def decode_views_device(self, blobs, indexes, views, parse_all=False, out=None):
        """mpc_decode_views_indexed_device: the same with the pixels left on the context's device.  out: a list of contiguous uint8
        torch tensors there, each of at least 3 * ceil(width / c) * ceil(height / c) elements of its view (bytes behind that are
        left alone); None = allocated here.  Returns (frames, routes), the frames uint8 tensors."""
        import torch
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        vw = self._views(views, n)
        if out is None:
            out = []
            for b, v in zip(bufs, vw):
                w, h = v.rect.width, v.rect.height
                if w == 0 and h == 0:
                    try:
                        w, h, _, _ = container_info(b)
                    except MpcError:                             # the call itself refuses the frame, in its turn, by its index
                        w, h = 1, 1
                c = 1 << min(max(v.scale_log2, 0), 3)
                out.append(torch.empty(3 * max(-(-w // c), 1) * max(-(-h // c), 1), dtype=torch.uint8, device=f"cuda:{self.device}"))
        if len(out) != n or any(t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() for t in out):
            raise ValueError("out: one contiguous uint8 device tensor per container")
        d_ptrs = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in out])
        caps = (C.c_size_t * n)(*[t.numel() for t in out])
        W, H, routes = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        torch.cuda.synchronize(self.device)                      # `out` may still be being written by the caller's streams
        _check(self.L.mpc_decode_views_indexed_device(self.h, ptrs, sizes, iptrs, isizes, vw, n, 1 if parse_all else 0, d_ptrs, caps, W, H,
                                                      routes))
        return [out[i].view(-1)[:3 * W[i] * H[i]].view(H[i], W[i], 3) for i in range(n)], list(routes)

    def transcode_views(self, blobs, indexes, views, parse_all=False):
        """mpc_transcode_views_indexed: transcode_container(blobs[f], views[f]) for every frame on the device -> (containers, routes):
        bytes objects, routes[f] 0 = through the frame's seek index (only the rectangle's window of the streams of the kept steps
        is parsed), 1 = the serial parse.  The container's K must be the context's.  parse_all: MPC_VIEW_PARSE_ALL."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes, n)
        vw = self._views(views, n)
        outs, nout, routes = (_u8p * n)(), (C.c_size_t * n)(), (C.c_int * n)()
        _check(self.L.mpc_transcode_views_indexed(self.h, ptrs, sizes, iptrs, isizes, vw, n, 1 if parse_all else 0, outs, nout, routes))
        return [_take_bytes(self.L, outs[i], C.c_size_t(nout[i])) for i in range(n)], list(routes)

    def crop_records_device(self, d_counts, d_choices, width, height, rect, steps, d_out_counts, d_out_choices, stream=0, check=True):
        """mpc_crop_records_device: whole-frame records of a width x height frame in device memory -> the records of the tile-aligned
        rectangle rect = (x, y, width, height) (None = the whole frame) as a frame of their own, counts cut to `steps` (0 = all), in
        d_out_counts[tiles' * 3] (uint16) and d_out_choices[tiles' * 3 * K] (uint32).  check: mpc_crop_records_check behind it, which
        waits for `stream` and raises MpcError(MPC_ERR_BITSTREAM) if a count above K was met."""
        rc = MpcRect(*[int(v) for v in (rect or (0, 0, 0, 0))])
        _check(self.L.mpc_crop_records_device(self.h, d_counts, d_choices, width, height, C.byref(rc), int(steps), d_out_counts, d_out_choices,
                                              stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def compose(self, blobs, indexes, parts, width, height, parse_all=False, index_interval=None, device_pixels=False):
        """mpc_compose_indexed: compose_container(blobs, parts, width, height) on the device, where a part's source may also be pixels
        (an HxWx3 uint8 array; with device_pixels a (data_ptr, width, height, row_stride) tuple of device memory), which stand for this
        context's encode of them with the destination's quantiser table -> (container, index or None, routes).  indexes: None, or one
        seek index (or None) per blob.  routes[p]: 0 = through the source's seek index, 1 = the serial parse, 2 = pixels, -1 = the part
        owns no tile and was skipped.  index_interval: None = no index, else container_index2(result, interval, expanded=True) comes
        with the container, from the entropy stage.  With no blobs the call is an encode from patches with the context's tables."""
        bufs, ptrs, sizes = self._containers(blobs)
        n = len(bufs)
        ibufs, iptrs, isizes = self._indexes(indexes if indexes is not None else [None] * n, n)
        made, keep = _parts(parts, device_pixels)
        flags = (1 if parse_all else 0) | (MPC_COMPOSE_DEVICE_PIXELS if device_pixels else 0)
        out, nout, index, nindex = _u8p(), C.c_size_t(0), _u8p(), C.c_size_t(0)
        routes = (C.c_int * len(made))()
        _check(self.L.mpc_compose_indexed(self.h, ptrs, sizes, iptrs, isizes, n, made, len(parts), int(width), int(height), flags,
                                          -1 if index_interval is None else int(index_interval), C.byref(out), C.byref(nout), C.byref(index),
                                          C.byref(nindex), routes))
        del keep, bufs, ibufs
        blob = _take_bytes(self.L, out, nout)
        return blob, None if index_interval is None else _take_bytes(self.L, index, nindex), list(routes)[:len(parts)]

    def paste_records_device(self, d_src_counts, d_src_choices, src_width, src_height, src_rect, d_dst_counts, d_dst_choices, dst_width,
                             dst_height, dst_x, dst_y, d_owner=None, part=0, stream=0, check=True):
        """mpc_paste_records_device: the records of the tile-aligned rectangle src_rect (None = the whole frame) of a src_width x
        src_height frame into the tiles at (dst_x, dst_y) of a dst_width x dst_height frame's records, both whole-frame records in device
        memory; counts min(count, K), records below the count copied, the steps behind them zero.  d_owner: None, or int32 per
        destination tile: only tiles with d_owner[t] == part are written.  check: mpc_crop_records_check behind it, which waits for
        `stream` and raises MpcError(MPC_ERR_BITSTREAM) if a count above K was met."""
        rc = MpcRect(*[int(v) for v in (src_rect or (0, 0, 0, 0))])
        _check(self.L.mpc_paste_records_device(self.h, d_src_counts, d_src_choices, int(src_width), int(src_height), C.byref(rc), d_dst_counts,
                                               d_dst_choices, int(dst_width), int(dst_height), int(dst_x), int(dst_y), d_owner or None, int(part),
                                               stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def _encode_cut(self, fn, info, result, frame, width, height, target, quant, index_interval, emphasis=()):
        """The call behind the budget and the quality encodes, their _device and their _emphasis forms: fn takes the frame, the map
        where `emphasis` holds one, the geometry, quant and the target (a budget in bytes, a squared error); info: the struct it fills;
        -> result(container, index, depth, info)"""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        tiles = -(-int(width) // 8) * -(-int(height) // 8)
        depth = np.zeros(max(tiles, 1), np.uint8)
        out, n, index, nindex, info = _u8p(), C.c_size_t(0), _u8p(), C.c_size_t(0), info()
        _check(fn(self.h, frame, *emphasis, int(width), int(height), qp, int(target), -1 if index_interval is None else int(index_interval),
                  C.byref(out), C.byref(n), C.byref(index), C.byref(nindex), depth.ctypes.data_as(_u8p), C.byref(info)))
        blob = _take_bytes(self.L, out, n)
        return result(blob, None if index_interval is None else _take_bytes(self.L, index, nindex), depth[:tiles], info)

    def _encode_budget(self, fn, frame, width, height, budget, quant, index_interval, emphasis=()):
        return self._encode_cut(fn, MpcBudgetInfo, BudgetResult, frame, width, height, budget, quant, index_interval, emphasis)

    def _encode_quality(self, fn, frame, width, height, psnr, max_sse, quant, index_interval, emphasis=()):
        if (psnr is None) == (max_sse is None):
            raise ValueError("exactly one of psnr and max_sse")
        if max_sse is None:
            max_sse = sse_for_psnr(psnr, width, height)
        return self._encode_cut(fn, MpcQualityInfo, QualityResult, frame, width, height, max_sse, quant, index_interval, emphasis)

    def encode_image_budget(self, rgb, budget, quant=None, index_interval=None):
        """mpc_encode_image_budget: the frame (uint8 [H, W, 3]) as a container of at most `budget` bytes, every tile cut to the depth that
        a Lagrange multiplier found by bisection assigns it -> BudgetResult.  index_interval: None = no index, else (0 = the default
        interval) container_index2(result, interval, expanded) comes with it."""
        rgb, W, H = _hwc_u8(rgb)
        return self._encode_budget(self.L.mpc_encode_image_budget, rgb.ctypes.data_as(C.c_void_p), W, H, budget, quant, index_interval)

    def encode_image_budget_device(self, d_rgb, width, height, budget, quant=None, index_interval=None):
        """The same with the frame in device memory (int from tensor.data_ptr(), tightly packed RGB)."""
        return self._encode_budget(self.L.mpc_encode_image_budget_device, C.c_void_p(int(d_rgb)), width, height, budget, quant, index_interval)

    def depth_profile_device(self, d_counts, d_choices, d_rgb, width, height, d_profile, quant=None, stream=0, check=True):
        """mpc_depth_profile_device: whole-frame records and the frame they came from (device pointers) -> d_profile[tiles, K + 1]
        (uint32): each tile's squared error with every count cut to n = 0 ... K.  check: mpc_crop_records_check behind it, which waits
        for `stream` and raises MpcError(MPC_ERR_BITSTREAM) if a record was not prefix-consistent or a count above K."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_depth_profile_device(self.h, d_counts, d_choices, qp, d_rgb, int(width), int(height), d_profile, stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def budget_allocate_device(self, d_profile, d_counts, tiles, weights, j, d_depth, d_out_counts, d_totals, stream=0):
        """mpc_budget_allocate_device: budget_allocate on the device; weights uint32 [3, K] in host memory; d_depth[tiles] (uint8),
        d_out_counts[tiles, 3] (uint16), d_totals[3] (uint64, zeroed first).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_allocate_device(self.h, d_profile, d_counts, int(tiles), weights.ctypes.data_as(_u32p), int(j), d_depth,
                                                 d_out_counts, d_totals, stream or None))

    def budget_sweep_device(self, d_profile, d_counts, tiles, weights, d_totals, stream=0):
        """mpc_budget_sweep_device: budget_sweep on the device, one launch for all 256 multipliers; weights uint32 [3, K] in host memory;
        d_totals[256, 3] (uint64, zeroed first).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_sweep_device(self.h, d_profile, d_counts, int(tiles), weights.ctypes.data_as(_u32p), d_totals, stream or None))

    def encode_image_quality(self, rgb, psnr=None, max_sse=None, quant=None, index_interval=None):
        """mpc_encode_image_quality: the frame (uint8 [H, W, 3]) as the container of the allocation at the largest multiplier whose
        squared error is at most the target -> QualityResult.  Exactly one target: psnr (dB; through sse_for_psnr) or max_sse.
        index_interval: as for encode_image_budget.  MpcError(MPC_ERR_ARGUMENT) where no cut of the frame's records is that good."""
        rgb, W, H = _hwc_u8(rgb)
        return self._encode_quality(self.L.mpc_encode_image_quality, rgb.ctypes.data_as(C.c_void_p), W, H, psnr, max_sse, quant, index_interval)

    def encode_image_quality_device(self, d_rgb, width, height, psnr=None, max_sse=None, quant=None, index_interval=None):
        """The same with the frame in device memory (int from tensor.data_ptr(), tightly packed RGB)."""
        return self._encode_quality(self.L.mpc_encode_image_quality_device, C.c_void_p(int(d_rgb)), width, height, psnr, max_sse, quant,
                                    index_interval)

    # ---- emphasis maps (include/mpcodec.h, "emphasis") ----
    def encode_image_budget_emphasis(self, rgb, budget, emphasis, quant=None, index_interval=None):
        """mpc_encode_image_budget_emphasis: encode_image_budget with an emphasis map (uint8 per tile, t = tx * tiles_y + ty; 16 =
        neutral, 1 ... 64) that weighs every tile's squared error in the allocation; None: encode_image_budget itself.  sse stays the
        true squared error of the result."""
        rgb, W, H = _hwc_u8(rgb)
        emphasis = _emphasis(emphasis, -(-W // 8) * -(-H // 8))
        return self._encode_budget(self.L.mpc_encode_image_budget_emphasis, rgb.ctypes.data_as(C.c_void_p), W, H, budget, quant, index_interval,
                                   (None if emphasis is None else C.c_void_p(emphasis.ctypes.data),))

    def encode_image_budget_emphasis_device(self, d_rgb, width, height, budget, d_emphasis, quant=None, index_interval=None):
        """The same with the frame and the map in device memory (ints from tensor.data_ptr(); d_emphasis 0 or None = neutral)."""
        return self._encode_budget(self.L.mpc_encode_image_budget_emphasis_device, C.c_void_p(int(d_rgb)), width, height, budget, quant,
                                   index_interval, (d_emphasis or None,))

    def encode_image_quality_emphasis(self, rgb, emphasis, psnr=None, max_sse=None, quant=None, index_interval=None):
        """mpc_encode_image_quality_emphasis: encode_image_quality with an emphasis map (as for encode_image_budget_emphasis).  The target
        stays a promise about the frame's true error; the map decides where the remaining error lies."""
        rgb, W, H = _hwc_u8(rgb)
        emphasis = _emphasis(emphasis, -(-W // 8) * -(-H // 8))
        return self._encode_quality(self.L.mpc_encode_image_quality_emphasis, rgb.ctypes.data_as(C.c_void_p), W, H, psnr, max_sse, quant,
                                    index_interval, (None if emphasis is None else C.c_void_p(emphasis.ctypes.data),))

    def encode_image_quality_emphasis_device(self, d_rgb, width, height, d_emphasis, psnr=None, max_sse=None, quant=None, index_interval=None):
        """The same with the frame and the map in device memory."""
        return self._encode_quality(self.L.mpc_encode_image_quality_emphasis_device, C.c_void_p(int(d_rgb)), width, height, psnr, max_sse,
                                    quant, index_interval, (d_emphasis or None,))

    # ---- a group of frames (include/mpcodec.h, "group") ----
    def _encode_group(self, fn, info_type, result, ptrs, emphasis, n, width, height, target, quant, index_interval):
        """The call behind encode_images_budget, encode_images_quality and their _device forms -> GroupResult"""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        tiles = -(-int(width) // 8) * -(-int(height) // 8)
        slots = max(n, 1)
        depth = np.zeros((slots, max(tiles, 1)), np.uint8)
        outs, sizes, idx, isizes = (_u8p * slots)(), (C.c_size_t * slots)(), (_u8p * slots)(), (C.c_size_t * slots)()
        frame_info, info = (info_type * slots)(), info_type()
        _check(fn(self.h, ptrs, emphasis, n, int(width), int(height), qp, int(target), -1 if index_interval is None else int(index_interval),
                  outs, sizes, idx, isizes, depth.ctypes.data_as(_u8p), frame_info, C.byref(info)))
        depth = depth.reshape(-1)[:n * tiles].reshape(n, tiles)
        frames = [result(_take_bytes(self.L, outs[f], C.c_size_t(sizes[f])),
                         None if index_interval is None else _take_bytes(self.L, idx[f], C.c_size_t(isizes[f])), depth[f], frame_info[f])
                  for f in range(n)]
        return GroupResult(frames, result(b"", None, None, info))

    @staticmethod
    def _host_group(frames, emphasis):
        """host frames of one size -> (the arrays, kept alive by the caller; their pointers; the map's pointer; n, W, H)"""
        frames = [_hwc_u8(f)[0] for f in frames]
        n = len(frames)
        H, W = frames[0].shape[:2] if n else (0, 0)
        if any(f.shape[:2] != (H, W) for f in frames):
            raise ValueError("frames must have the same size")
        emphasis = _emphasis(emphasis, n * -(-W // 8) * -(-H // 8))
        ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(f.ctypes.data) for f in frames])
        return frames, emphasis, ptrs, None if emphasis is None else C.c_void_p(emphasis.ctypes.data), n, W, H

    @staticmethod
    def _device_group(d_frames):
        n = len(d_frames)
        return (C.c_void_p * max(n, 1))(*[C.c_void_p(int(p) or None) for p in d_frames]), n

    def encode_images_budget(self, frames, budget, emphasis=None, quant=None, index_interval=None):
        """mpc_encode_images_budget: equally sized host frames (uint8 [H, W, 3] each, 1 ... 64 of them) as containers of at most `budget`
        bytes together, one Lagrange multiplier across all tiles of all frames -> GroupResult of BudgetResults.  emphasis: None or uint8
        [frames, tiles]; index_interval: as for encode_image_budget.  One frame: encode_image_budget's result."""
        keep, emphasis, ptrs, ep, n, W, H = self._host_group(frames, emphasis)
        return self._encode_group(self.L.mpc_encode_images_budget, MpcBudgetInfo, BudgetResult, ptrs, ep, n, W, H, budget, quant, index_interval)

    def encode_images_budget_device(self, d_frames, width, height, budget, d_emphasis=None, quant=None, index_interval=None):
        """The same with the frames (ints from tensor.data_ptr(), tightly packed RGB) and the map (0 or None = none) in device memory."""
        ptrs, n = self._device_group(d_frames)
        return self._encode_group(self.L.mpc_encode_images_budget_device, MpcBudgetInfo, BudgetResult, ptrs, d_emphasis or None, n, width, height,
                                  budget, quant, index_interval)

    def _group_target(self, psnr, max_sse, width, height, n):
        if (psnr is None) == (max_sse is None):
            raise ValueError("exactly one of psnr and max_sse")
        return sse_for_psnr_group(psnr, width, height, n) if max_sse is None else max_sse

    def encode_images_quality(self, frames, psnr=None, max_sse=None, emphasis=None, quant=None, index_interval=None):
        """mpc_encode_images_quality: equally sized host frames as the containers of the group allocation at the largest multiplier whose
        squared error over the whole group is at most the target -> GroupResult of QualityResults.  Exactly one target: psnr (dB over
        all the frames' pixels; through sse_for_psnr_group) or max_sse (the group's total).  One frame: encode_image_quality's result."""
        keep, emphasis, ptrs, ep, n, W, H = self._host_group(frames, emphasis)
        return self._encode_group(self.L.mpc_encode_images_quality, MpcQualityInfo, QualityResult, ptrs, ep, n, W, H,
                                  self._group_target(psnr, max_sse, W, H, n), quant, index_interval)

    def encode_images_quality_device(self, d_frames, width, height, psnr=None, max_sse=None, d_emphasis=None, quant=None, index_interval=None):
        """The same with the frames and the map in device memory."""
        ptrs, n = self._device_group(d_frames)
        return self._encode_group(self.L.mpc_encode_images_quality_device, MpcQualityInfo, QualityResult, ptrs, d_emphasis or None, n, width,
                                  height, self._group_target(psnr, max_sse, width, height, n), quant, index_interval)

    def budget_allocate_group_device(self, d_profile, d_counts, d_emphasis, frames, tiles, weights, j, d_depth, d_out_counts, d_totals, stream=0):
        """mpc_budget_allocate_group_device: budget_allocate_group on the device; weights uint32 [frames, 3, K] in host memory; d_emphasis
        0 = none; d_depth[frames * tiles] (uint8), d_out_counts[frames * tiles * 3], d_totals[frames * 3] (uint64).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(-1, 3, self.K)
        if weights.shape[0] != frames and 1 <= frames <= MPC_GROUP_MAX_FRAMES:
            raise ValueError(f"weights of {weights.shape[0]} frames for {frames}")
        _check(self.L.mpc_budget_allocate_group_device(self.h, d_profile, d_counts, d_emphasis or None, int(frames), int(tiles),
                                                       weights.ctypes.data_as(_u32p), int(j), d_depth, d_out_counts, d_totals, stream or None))

    def budget_sweep_group_device(self, d_profile, d_counts, d_emphasis, frames, tiles, weights, d_totals, stream=0):
        """mpc_budget_sweep_group_device: budget_sweep_group on the device, all 256 multipliers and all frames; d_totals[768] (uint64).
        Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(-1, 3, self.K)
        if weights.shape[0] != frames and 1 <= frames <= MPC_GROUP_MAX_FRAMES:
            raise ValueError(f"weights of {weights.shape[0]} frames for {frames}")
        _check(self.L.mpc_budget_sweep_group_device(self.h, d_profile, d_counts, d_emphasis or None, int(frames), int(tiles),
                                                    weights.ctypes.data_as(_u32p), d_totals, stream or None))

    def budget_allocate_emphasis_device(self, d_profile, d_counts, d_emphasis, tiles, weights, j, d_depth, d_out_counts, d_totals, stream=0):
        """mpc_budget_allocate_emphasis_device: budget_allocate_device with d_emphasis[tiles] (uint8; 0 = neutral).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_allocate_emphasis_device(self.h, d_profile, d_counts, d_emphasis or None, int(tiles), weights.ctypes.data_as(_u32p),
                                                          int(j), d_depth, d_out_counts, d_totals, stream or None))

    def budget_sweep_emphasis_device(self, d_profile, d_counts, d_emphasis, tiles, weights, d_totals, stream=0):
        """mpc_budget_sweep_emphasis_device: budget_sweep_device with d_emphasis[tiles] (uint8; 0 = neutral).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_sweep_emphasis_device(self.h, d_profile, d_counts, d_emphasis or None, int(tiles), weights.ctypes.data_as(_u32p),
                                                       d_totals, stream or None))

    def budget_allocate_floor_emphasis_device(self, d_profile, d_counts, d_floor, d_must, d_emphasis, d_list, tiles, n, weights, j, d_depth,
                                              d_out_counts, d_send, d_totals, stream=0):
        """mpc_budget_allocate_floor_emphasis_device: budget_allocate_floor_device with the frame's d_emphasis[tiles] (uint8; 0 = neutral)
        and d_list[n] (int32: candidate -> tile; 0 = the identity).  Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_allocate_floor_emphasis_device(self.h, d_profile, d_counts, d_floor or None, d_must or None, d_emphasis or None,
                                                                d_list or None, int(tiles), int(n), weights.ctypes.data_as(_u32p), int(j),
                                                                d_depth, d_out_counts, d_send, d_totals, stream or None))

    def emphasis_from_mask_device(self, d_mask, width, height, d_emphasis, lo=1, hi=MPC_EMPHASIS_MAX, row_stride=0, stream=0):
        """mpc_emphasis_from_mask_device: emphasis_from_mask on the device: d_mask (uint8, row_stride bytes a row, 0 = width; a torch
        tensor's data_ptr()) -> d_emphasis[tiles].  Asynchronous."""
        _check(self.L.mpc_emphasis_from_mask_device(self.h, d_mask or None, int(width), int(height), int(row_stride) or int(width), int(lo),
                                                    int(hi), d_emphasis or None, stream or None))

    def owed_tiles_device(self, d_sent, d_counts, tiles, d_flags, d_floor, d_must, d_list, d_count, stream=0):
        """mpc_owed_tiles_device: d_flags[tiles] (uint8, != 0: changed) gains the owed tiles of d_sent / d_counts; d_floor and d_must
        per tile as owed_tiles gives them; the candidates, ascending, in d_list (int32 per tile) and d_count (int32).  Asynchronous."""
        _check(self.L.mpc_owed_tiles_device(self.h, d_sent, d_counts, int(tiles), d_flags, d_floor, d_must, d_list, d_count, stream or None))

    def gather_records_device(self, d_counts, d_choices, tiles, d_list, m, d_idx, d_depth, n, rows, d_packed_counts, d_packed_choices,
                              stream=0, check=True):
        """mpc_gather_records_device: scatter_records_device turned round: packed tile j < n of delta_pack_geometry(n, rows) takes the
        records of tile d_list[d_idx[j]] (d_idx 0 = the identity) cut to d_depth[d_idx[j]] (0 = uncut), zero above the cut and in the
        padding tiles.  check: mpc_crop_records_check behind it, which waits for `stream` and raises MpcError(MPC_ERR_BITSTREAM) if an
        entry was outside its range (that packed tile is all zero)."""
        _check(self.L.mpc_gather_records_device(self.h, d_counts, d_choices, int(tiles), d_list, int(m), d_idx or None, d_depth or None, int(n),
                                                int(rows), d_packed_counts, d_packed_choices, stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def budget_allocate_floor_device(self, d_profile, d_counts, d_floor, d_must, n, weights, j, d_depth, d_out_counts, d_send, d_totals,
                                     stream=0):
        """mpc_budget_allocate_floor_device: budget_allocate_floor on the device; weights uint32 [3, K] in host memory; d_floor, d_must
        (uint8 [n]; 0 = all 0, all 1); d_depth[n], d_send[n] (uint8), d_out_counts[n, 3] (uint16), d_totals[4] (uint64, zeroed first).
        Asynchronous."""
        weights = np.ascontiguousarray(weights, np.uint32).reshape(3, self.K)
        _check(self.L.mpc_budget_allocate_floor_device(self.h, d_profile, d_counts, d_floor or None, d_must or None, int(n),
                                                       weights.ctypes.data_as(_u32p), int(j), d_depth, d_out_counts, d_send, d_totals,
                                                       stream or None))

    def delta_encoder(self, width, height):
        """mpc_delta_create: a DeltaEncoder for frames of width x height through this context"""
        return DeltaEncoder(self, width, height)

    def tile_diff_device(self, d_kept, d_rgb, width, height, row_stride, d_list, d_count, stream=0):
        """mpc_tile_diff_device: the 8 x 8 tiles of the frame at d_rgb (row_stride bytes between rows, 0 = 3 * width) that differ from the
        tight copy at d_kept -> d_list (int32 per tile, ascending) and d_count (int32); d_kept becomes the new pixels.  Asynchronous."""
        _check(self.L.mpc_tile_diff_device(self.h, d_kept, d_rgb, int(width), int(height), int(row_stride), d_list, d_count, stream or None))

    def tile_diff_tolerance_device(self, d_kept, d_rgb, width, height, row_stride, tolerance, d_list, d_count, d_sse=0, stream=0):
        """mpc_tile_diff_tolerance_device: tile_diff_device with a tolerance -- d_list / d_count the tiles whose summed squared byte
        difference exceeds it; d_kept becomes the new pixels in those tiles only; d_sse (0 = none): uint32 per tile.  Asynchronous."""
        _check(self.L.mpc_tile_diff_tolerance_device(self.h, d_kept, d_rgb, int(width), int(height), int(row_stride), int(tolerance), d_list,
                                                     d_count, d_sse or None, stream or None))

    def pack_tiles_device(self, d_rgb, width, height, row_stride, d_list, n, rows, d_packed, packed_stride=0, stream=0):
        """mpc_pack_tiles_device: the n listed tiles of the frame as the packed frame delta_pack_geometry(n, rows) describes, black
        outside the image and in the padding tiles.  Asynchronous."""
        _check(self.L.mpc_pack_tiles_device(self.h, d_rgb, int(width), int(height), int(row_stride), d_list, int(n), int(rows), d_packed,
                                            int(packed_stride), stream or None))

    def patch_decoder(self, width, height):
        """mpc_patch_decoder_create: a PatchDecoder for a delta stream of width x height frames through this context"""
        return PatchDecoder(self, width, height)

    def unpack_tiles_device(self, d_packed, packed_stride, d_list, n, rows, d_rgb, width, height, row_stride=0, stream=0, check=True):
        """mpc_unpack_tiles_device: pack_tiles_device's inverse: listed tile j of the packed frame delta_pack_geometry(n, rows) describes to
        tile d_list[j] of the frame at d_rgb, only the bytes inside the image.  check: mpc_crop_records_check behind it, which waits for
        `stream` and raises MpcError(MPC_ERR_BITSTREAM) if a list entry was outside the frame (that entry writes nothing)."""
        _check(self.L.mpc_unpack_tiles_device(self.h, d_packed, int(packed_stride), d_list, int(n), int(rows), d_rgb, int(width), int(height),
                                              int(row_stride), stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def scatter_records_device(self, d_packed_counts, d_packed_choices, d_list, n, d_counts, d_choices, tiles, stream=0, check=True):
        """mpc_scatter_records_device: records j of a packed frame to tile d_list[j] of whole-frame records of `tiles` tiles.  check:
        mpc_crop_records_check behind it, which waits for `stream` and raises MpcError(MPC_ERR_BITSTREAM) if a list entry was outside
        [0, tiles) (that entry is skipped)."""
        _check(self.L.mpc_scatter_records_device(self.h, d_packed_counts, d_packed_choices, d_list, int(n), d_counts, d_choices, int(tiles),
                                                 stream or None))
        if check:
            _check(self.L.mpc_crop_records_check(self.h, stream or None))

    def parse_container_view_device(self, blob, index, view, parse_all=False):
        """mpc_parse_container_view_device: parse_container_view_by_index with the device's lengths parse, lengths cut, ranks,
        windowed parse and windowed unpack -> (symbols, ranges, route)."""
        buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
        return _view_parse(self.L.mpc_parse_container_view_device, (self.h,), buf, idx, view, parse_all)

    def parse_container_window_device(self, blob, index, rect, parse_all=False):
        """mpc_parse_container_window_device: parse_container_window_by_index with the device's lengths parse, ranks, windowed
        parse and windowed unpack -> (symbols, ranges, route)."""
        buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
        return _window_parse(self.L.mpc_parse_container_window_device, (self.h,), buf, idx, rect, parse_all)

    def window_chunks_device(self, blob, index, rect, parse_all=False):
        """mpc_window_chunks_device: window_chunks_by_index as the device's rank kernel writes it -> (chunks[6K, 2], route)"""
        return _window_chunks(self.L.mpc_window_chunks_device, (self.h,), blob, index, rect, parse_all)

    def parse_container_device(self, blob, index):
        """mpc_parse_container_device: parse_container_by_index with the chunks decoded on the device (the decoder's own
        upload-and-parse step) -> (symbols, route)."""
        buf, idx = np.frombuffer(blob, np.uint8), np.frombuffer(index, np.uint8)
        out, n, route = _u16p(), C.c_size_t(0), C.c_int(-1)
        _check(self.L.mpc_parse_container_device(self.h, buf.ctypes.data_as(_u8p), buf.size, idx.ctypes.data_as(_u8p), idx.size,
                                                 C.byref(out), C.byref(n), C.byref(route)))
        return _take_u16(self.L, out, n), route.value

    def unpack_symbol_streams_device(self, coded, packed, expect):
        """mpc_unpack_symbol_streams_device: coded[6K] = the streams as entropy-decoded, packed[6K] = run-length packed or not,
        expect[6K] = the symbols each must expand to -> all streams expanded and the step-0 coefficient streams summed, back to
        back (uint16); MpcError(MPC_ERR_BITSTREAM) when a stream does not expand to exactly expect[i] symbols."""
        K = len(coded) // 6                                      # the streams' own K, not the context's
        symbols, off = _symbol_streams(K, coded)
        flags = np.ascontiguousarray(packed, np.uint8)
        want = np.ascontiguousarray(expect, np.uint64)
        assert flags.size == 6 * K and want.size == 6 * K
        out, n = _u16p(), C.c_size_t(0)
        _check(self.L.mpc_unpack_symbol_streams_device(self.h, K, symbols.ctypes.data_as(_u16p),
                                                       off.ctypes.data_as(C.POINTER(C.c_ulonglong)), flags.ctypes.data_as(_u8p),
                                                       want.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(out), C.byref(n)))
        return _take_u16(self.L, out, n)

    def interleave_stripe_device(self, d_part_counts, d_part_choices, width, height, tile_row_begin, tile_row_end, d_frame_counts,
                                 d_frame_choices, stream=0):
        """mpc_interleave_stripe_device: a row stripe's records (stripe order) -> their places in the whole frame's records."""
        _check(self.L.mpc_interleave_stripe_device(self.h, d_part_counts, d_part_choices, width, height, tile_row_begin, tile_row_end,
                                                   d_frame_counts, d_frame_choices, stream or None))

    def records_to_container_device(self, d_counts, d_choices, width, height, quant=None, stream=0):
        """mpc_records_to_container_device: whole-frame records in device memory -> container bytes."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        out, n = _u8p(), C.c_size_t(0)
        _check(self.L.mpc_records_to_container_device(self.h, d_counts, d_choices, width, height, qp, stream or None, C.byref(out), C.byref(n)))
        return _take_bytes(self.L, out, n)

    def code_symbol_streams_device(self, width, height, counts, streams, quant=None):
        """mpc_code_symbol_streams_device: assembled streams (host) -> container bytes with the per-symbol work of the entropy
        stage on the device.  Returns (bytes, route): route 0 = device, 1 = the host route was taken."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        cn, cp = _u16(counts)
        symbols, off = _symbol_streams(self.K, streams)
        out, n, route = _u8p(), C.c_size_t(0), C.c_int(-1)
        _check(self.L.mpc_code_symbol_streams_device(self.h, width, height, qp, cp, symbols.ctypes.data_as(_u16p),
                                                     off.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(out), C.byref(n), C.byref(route)))
        return _take_bytes(self.L, out, n), route.value

    def code_symbol_streams_device_indexed(self, width, height, counts, streams, interval=0, quant=None, expanded=False):
        """mpc_code_symbol_streams_device_indexed: code_symbol_streams_device with the container's seek index ->
        (container, index or None, route); None for streams that do not hold what `counts` implies.  expanded: index version 2
        (mpc_code_symbol_streams_device_indexed2 with MPC_INDEX_EXPANDED)."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        cn, cp = _u16(counts)
        symbols, off = _symbol_streams(self.K, streams)
        out, n, idx, ni, route = _u8p(), C.c_size_t(0), _u8p(), C.c_size_t(0), C.c_int(-1)
        head = (self.h, width, height, qp, cp, symbols.ctypes.data_as(_u16p), off.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(interval))
        tail = (C.byref(out), C.byref(n), C.byref(idx), C.byref(ni), C.byref(route))
        if expanded:
            _check(self.L.mpc_code_symbol_streams_device_indexed2(*head, MPC_INDEX_EXPANDED, *tail))
        else:
            _check(self.L.mpc_code_symbol_streams_device_indexed(*head, *tail))
        return _take_bytes(self.L, out, n), (_take_bytes(self.L, idx, ni) if idx else None), route.value

    def decode_tiles_device(self, d_counts, d_choices, width, height, d_rgb, quant=None, stream=0):
        """mpc_decode_tiles_device: whole-frame records in device memory -> d_rgb[height, width, 3] (uint8), reconstructed with `quant`
        (None = the context's tables) exactly as given, not truncated to the container header's u16.  Asynchronous on `stream`."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_decode_tiles_device(self.h, d_counts, d_choices, qp, int(width), int(height), d_rgb, stream or None))

    def container_job_begin(self, slot, d_counts, d_choices, width, height, quant=None, stream=0):
        """mpc_container_job_begin: stream assembly + entropy phase 1 of whole-frame records in device memory, enqueued only."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_container_job_begin(self.h, slot, d_counts, d_choices, width, height, qp, stream or None))

    def container_job_tables(self, slot):
        """mpc_container_job_tables: wait for phase 1, build the code tables, enqueue phase 2 and the container's copy."""
        _check(self.L.mpc_container_job_tables(self.h, slot))

    def container_job_collect(self, slot, views=False):
        """mpc_container_job_collect: wait for the copy -> container bytes (views=True: a uint8 array on the library's buffer)."""
        out, n = _u8p(), C.c_size_t(0)
        _check(self.L.mpc_container_job_collect(self.h, slot, C.byref(out), C.byref(n)))
        return (_take_view if views else _take_bytes)(self.L, out, n)

    def container_job_cancel(self, slot):
        """mpc_container_job_cancel: give the slot up whatever step its job is at."""
        _check(self.L.mpc_container_job_cancel(self.h, slot))

    # -- rate-distortion sweep (Compression.cpp -n / -g) ------------------------------------------
    def _rate_distortion(self, fn, frame, width, height, qualities, keep_bytes):
        labels, quants = parse_qualities(qualities, self.K, self.block_size)
        n = len(labels)
        sizes = (C.c_size_t * n)()
        sse = np.zeros(n, np.uint64)
        psnr = np.zeros(n, np.float64)
        outs = (_u8p * n)() if keep_bytes else None
        _check(fn(self.h, frame, int(width), int(height), quants.ctypes.data_as(_dp), n, sizes,
                  sse.ctypes.data_as(C.POINTER(C.c_ulonglong)), psnr.ctypes.data_as(_dp), outs))
        pixels = float(int(width) * int(height))
        points = []
        for i in range(n):
            blob = _take_bytes(self.L, outs[i], C.c_size_t(sizes[i])) if keep_bytes else None
            points.append(RatePoint(labels[i], quants[i], int(sizes[i]), float(8 * int(sizes[i])) / pixels, int(sse[i]),
                                    float(psnr[i]), blob))
        return points

    def rate_distortion(self, rgb, qualities, keep_bytes=False):
        """mpc_rate_distortion: one frame (uint8 [H, W, 3]) at every level of `qualities` (see parse_qualities) -> a list of
        RatePoint: per level the container's size (the container itself with keep_bytes), bpp, the exact squared error against
        what decode_image would reconstruct and its PSNR (bit-equal to calculate_psnr)."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        H, W = rgb.shape[:2]
        return self._rate_distortion(self.L.mpc_rate_distortion, rgb.ctypes.data_as(C.c_void_p), W, H, qualities, keep_bytes)

    def rate_distortion_device(self, d_rgb, width, height, qualities, keep_bytes=False):
        """mpc_rate_distortion_device: the same with the frame in device memory (int from tensor.data_ptr(), tightly packed RGB)."""
        return self._rate_distortion(self.L.mpc_rate_distortion_device, C.c_void_p(int(d_rgb)), width, height, qualities, keep_bytes)

    def distortion_device(self, d_counts, d_choices, d_rgb, width, height, d_sse, d_tile_sse=None, quant=None, stream=0):
        """mpc_distortion_device: whole-frame records and the frame they came from (device pointers) -> *d_sse (u64) += the squared
        error of the decoder's reconstruction (quant truncated to u16 as the container carries it); d_tile_sse: per tile (u32)."""
        qp = None
        if quant is not None:
            quant = np.ascontiguousarray(quant, np.float64).reshape(3, self.K)
            qp = quant.ctypes.data_as(_dp)
        _check(self.L.mpc_distortion_device(self.h, d_counts, d_choices, qp, d_rgb, width, height, d_sse, d_tile_sse or None,
                                            stream or None))

    # -- the tests' entry points to the screen's tables -------------------------------------------
    def debug_copy_gram_device(self, channel, sel_begin, sel_count, col_begin, col_count, d_out, stream=0):
        """mpc_debug_copy_gram_device: a rectangle of the resident Gram table of `channel` -> dense float32 d_out[sel_count, col_count]."""
        _check(self.L.mpc_debug_copy_gram_device(self.h, int(channel), int(sel_begin), int(sel_count), int(col_begin), int(col_count),
                                                 d_out or None, stream or None))

    def debug_copy_filter_tiles(self, channel, block=0):
        """mpc_debug_copy_filter_tiles: the uploaded tiles as uint16: the 32 base tiles (channel -1) or the 4 of (channel, block)."""
        out = np.zeros((32 if channel < 0 else 4) * FILTER_TILE_HALVES, np.uint16)
        _check(self.L.mpc_debug_copy_filter_tiles(self.h, int(channel), int(block), out.ctypes.data_as(_u16p)))
        return out

    def debug_screen_probe_device(self, channel, block, d_vectors, n, d_approx, d_bound, stream=0):
        """mpc_debug_screen_probe_device: d_vectors[n,64] f64 -> d_approx[n,576] f32 (base rows 0..511, block rows 0..63), d_bound[n]."""
        _check(self.L.mpc_debug_screen_probe_device(self.h, int(channel), int(block), d_vectors or None, int(n), d_approx or None,
                                                    d_bound or None, stream or None))

    def debug_track_probe_device(self, d_row_bits, d_pair_bits, bound, rows, pair, d_out, stream=0):
        """mpc_debug_track_probe_device: d_row_bits[64,144] u32, d_pair_bits[64,16] u32 -> d_out[64,14] u32: the keys of the kernel's
        tracking, by the definition and grouped (base, block, pair with the largest |P|)."""
        _check(self.L.mpc_debug_track_probe_device(self.h, d_row_bits or None, d_pair_bits or None, float(bound), int(rows), int(pair),
                                                   d_out or None, stream or None))

    def debug_pair_scratch(self, wave_begin, wave_count, fill_word=None):
        """mpc_debug_pair_scratch: the pursuit kernel's pair scratch of waves [wave_begin, + wave_count), every 32-bit word set to
        `fill_word` first if one is given -> P float32[waves,16,32,64], meta uint32[waves,16,32,2], E float32[waves,16,32]."""
        n = max(int(wave_count), 1)
        p = np.zeros((n, 16, PAIR_SCRATCH_PAIRS, 64), np.float32)
        meta = np.zeros((n, 16, PAIR_SCRATCH_PAIRS, 2), np.uint32)
        e = np.zeros((n, 16, PAIR_SCRATCH_PAIRS), np.float32)
        _check(self.L.mpc_debug_pair_scratch(self.h, int(wave_begin), int(wave_count), 0 if fill_word is None else 1,
                                             int(fill_word or 0), p.ctypes.data, meta.ctypes.data, e.ctypes.data))
        return p, meta, e

    def calc_mp(self, channel, vectors, quant_k=None):
        """matching::CalcMPDynamic (MatchingPursuit.h:22) on the device for vectors[n,64].
        Returns counts[n], choices[n,K], energy[n], swept[n]."""
        v = np.ascontiguousarray(vectors, np.float64).reshape(-1, 64)
        n = v.shape[0]
        counts = np.zeros(n, np.uint16)
        choices = np.zeros((n, self.K), CHOICE_DTYPE)
        energy = np.zeros(n)
        swept = np.zeros(n, np.uint32)
        qp = None
        if quant_k is not None:
            quant_k = np.ascontiguousarray(quant_k, np.float64)
            qp = quant_k.ctypes.data_as(_dp)
        _check(self.L.mpc_calc_mp_batch(self.h, channel, qp, v.ctypes.data_as(_dp), n,
                                        choices.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(_u16p),
                                        energy.ctypes.data_as(_dp), swept.ctypes.data_as(_u32p)))
        return counts, choices, energy, swept


FILTER_TILE_HALVES = 2048          # 16-bit elements of one filter tile (16 rows x 64 pixels, hi and lo)
PAIR_SCRATCH_PAIRS = 32            # pairs a slot of the pursuit kernel can hold (mp_device.h: kMaxPairs)


def filter_tiles(rows, tiles, k_order=0):
    """mpc_filter_tiles (host only, for the tests): rows[nrows,64] doubles -> (out uint16[tiles * 2048], shadow uint8[nrows])."""
    L = load_library()
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 64)
    out = np.full(int(tiles) * FILTER_TILE_HALVES if tiles > 0 else 1, 0xFFFF, np.uint16)
    shadow = np.full(max(rows.shape[0], 1), 0xFF, np.uint8)
    _check(L.mpc_filter_tiles(rows.ctypes.data_as(_dp), rows.shape[0], int(tiles), int(k_order), out.ctypes.data_as(_u16p),
                              shadow.ctypes.data_as(_u8p)))
    return out, shadow[:rows.shape[0]]


def debug_gram_device(d_base, d_detail, d_block_rows, d_block_row_off, d_shadow, num_base, n_sel, d_gram, stream=0):
    """mpc_debug_gram_device (for the tests): the Gram kernel on the caller's own device arrays (ints from tensor.data_ptr())."""
    _check(load_library().mpc_debug_gram_device(d_base or None, d_detail or None, d_block_rows or None, d_block_row_off or None,
                                                d_shadow or None, int(num_base), int(n_sel), d_gram or None, stream or None))


def encode_images_multi(contexts, frames, quant=None, views=False):
    """mpc_encode_images_multi: frames (host, equal sizes) through several contexts, one per device lane: every frame's tile rows
    striped over the lanes, the stripes pulled to the frame's owner, one container per frame (byte-identical to encode_image)."""
    L = load_library()
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    H, W = frames[0].shape[:2]
    if any(f.shape[:2] != (H, W) for f in frames):
        raise ValueError("frames must have the same size")
    K = contexts[0].K
    qp = None
    if quant is not None:
        quant = np.ascontiguousarray(quant, np.float64).reshape(3, K)
        qp = quant.ctypes.data_as(_dp)
    n = len(frames)
    handles = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    ptrs = (_u8p * n)(*[f.ctypes.data_as(_u8p) for f in frames])
    outs = (_u8p * n)()
    sizes = (C.c_size_t * n)()
    _check(L.mpc_encode_images_multi(handles, len(contexts), ptrs, n, W, H, qp, outs, sizes))
    take = _take_view if views else _take_bytes
    return [take(L, outs[i], C.c_size_t(sizes[i])) for i in range(n)]


def create_compression_context(K=32, block_size=8, bpp=3.5, device=-1):
    """compressed::createCompressionContext(K, blockSize, bppAllocation) (CompressedImage.h:54)."""
    return CompressionContext(K, block_size, bpp, device)
