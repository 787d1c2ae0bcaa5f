"""ctypes binding of the C ABI in include/cloudini_hip.h (cloudini_amd/lib/libcloudini_hip.so).

This is the product path's only entry to the HIP kernels from Python (tests, bench.py, smoke). It fails
loudly when the library has not been built or when no GPU is present -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.environ.get("CLDN_HIP_LIB_OVERRIDE") or os.path.join(HERE, "lib", "libcloudini_hip.so")  # override: A/B builds

HOST, DEVICE = 0, 1
STAGE2_NONE, STAGE2_LZ4, STAGE2_LZ4_FAST, STAGE2_ZSTD = 0, 1, 2, 3   # cldn_hip_codec_set_stage2

ERRORS = {-1: "ARG", -2: "CAPACITY", -3: "UNSUPPORTED", -4: "DEVICE", -5: "NO_DEVICE", -6: "CORRUPT", -7: "NOMEM"}


class _Segment(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32)]


class ChunkTable(C.Structure):
    """cldn_hip_chunk_table_t: device pointers into the codec's workspace (valid until the codec's next call)."""
    _fields_ = [("payload_base", C.c_void_p), ("chunk_stride", C.c_uint64), ("segments", C.c_void_p),
                ("segments_per_chunk", C.c_uint32), ("n_chunks", C.c_uint32), ("chunk_sizes", C.c_void_p),
                ("not_contiguous", C.c_void_p)]


class CloudiniHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"cloudini_hip error {code} ({ERRORS.get(code, '?')}): {message}")
        self.code = code
        self.message = message


class _Field(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("type", C.c_uint8), ("has_resolution", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("resolution", C.c_float)]


_INT, _U8, _U32, _U64, _I64, _F32 = C.c_int, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int64, C.c_float
_VP, _U8P, _U32P, _U64P, _F32P, _VPP = (C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_float), C.POINTER(C.c_void_p))

# name -> (restype, argtypes) of every prototype of include/cloudini_hip.h, in its order, and of the debug hooks hip_abi.hip
# exports outside it. lib() applies the table; tests/test_host_api.py holds it against the C declarations.
SIGNATURES = {
    "cldn_hip_last_error": (C.c_char_p, []),
    "cldn_hip_abi_version": (_INT, []),
    "cldn_hip_device_count": (_INT, []),
    "cldn_hip_current_device": (_INT, []),
    "cldn_hip_set_current_device": (_INT, [_INT]),
    "cldn_hip_host_alloc": (_VP, [C.c_size_t]),
    "cldn_hip_host_free": (None, [_VP]),
    "cldn_hip_plan_create": (_INT, [C.POINTER(_Field), _U32, _U32, _U8, _U8, _VPP]),
    "cldn_hip_plan_destroy": (None, [_VP]),
    "cldn_hip_plan_uses_v5": (_INT, [_VP]),
    "cldn_hip_plan_adaptive_fields": (_U32, [_VP]),
    "cldn_hip_plan_adaptive_field_index": (_U32, [_VP, _U32]),
    "cldn_hip_plan_max_point_bytes": (_U32, [_VP]),
    "cldn_hip_stage1_bound": (_U64, [_VP, _U64]),
    "cldn_hip_codec_create": (_INT, [_VP, _INT, _VP, _VPP]),
    "cldn_hip_codec_destroy": (None, [_VP]),
    "cldn_hip_codec_synchronize": (_INT, [_VP]),
    "cldn_hip_codec_stream": (_VP, [_VP]),
    "cldn_hip_codec_device": (_INT, [_VP]),
    "cldn_hip_encode_stage1": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _U64, _INT, _VP, _VP, _VP]),
    "cldn_hip_encode_stage1_chunks": (_INT, [_VP, _VP, _INT, _U64P, _U32, C.POINTER(ChunkTable), _VP]),
    "cldn_hip_frame_chunks": (_INT, [_VP, _VP, _U64, _INT, _VP, _VP]),
    "cldn_hip_codec_fetch_output": (_INT, [_VP, _VP, _U64]),
    "cldn_hip_encode_stage1_gather": (_INT, [_VP, _VPP, _U64P, _U32, _VP, _U64, _INT, _VP, _VP, _VP]),
    "cldn_hip_codec_set_stage2": (_INT, [_VP, _INT]),
    "cldn_hip_stage2_bound": (_U64, [_VP, _U64, _INT]),
    "cldn_hip_codec_force_modes": (_INT, [_VP, _U8P, _U32]),
    "cldn_hip_codec_force_modes_per_cloud": (_INT, [_VP, _U8P, _U32]),
    "cldn_hip_codec_pipeline": (_INT, [_VP, _INT, _VP]),
    "cldn_hip_decode_stage1": (_INT, [_VP, _VP, _INT, _U64P, _U64P, _U32, _VP, _U64, _INT]),
    "cldn_hip_decode_stage1_sized": (_INT, [_VP, _VP, _INT, _U64P, _U64P, _U32, _VP, _INT, _VP, _U64, _INT]),
    "cldn_hip_lz4_decompress": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _INT, _U64P, _VP]),
    "cldn_hip_decode_lz4": (_INT, [_VP, _VP, _INT, _U64P, _U64P, _U32, _VP, _U64, _INT]),
    "cldn_hip_zstd_decompress": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _INT, _U64P, _VP]),
    "cldn_hip_decode_zstd": (_INT, [_VP, _VP, _INT, _U64P, _U64P, _U32, _VP, _U64, _INT]),
    "cldn_hip_decode_lz4_gather": (_INT, [_VP, _VP, _U64P, _U64P, _U32, _VP, _VP, _VP, _VP, _VP, _U64, _INT]),
    "cldn_hip_decode_zstd_gather": (_INT, [_VP, _VP, _U64P, _U64P, _U32, _VP, _VP, _VP, _VP, _VP, _U64, _INT]),
    "cldn_hip_decode_stage1_unframed": (_INT, [_VP, _VP, _U64, _INT, _VP, _U64, _INT]),
    "cldn_hip_viz_preprocess": (_INT, [_VP, _VP, _INT, _U64, _U32, _U32, _F32, _VP, _U64, _INT, _U64P]),
    "cldn_hip_viz_preprocess_batch": (_INT, [_VP, _VP, _INT, _U64P, _U32, _U32, _U32, _F32, _VP, _U64, _INT, _U64P]),
    "cldn_hip_encode_stage1_viz": (_INT, [_VP, _VP, _INT, _U64P, _U32, _U32, _F32, _U64P, _VP, _U64, _INT, _VP, _VP, _VP]),
    "cldn_hip_encode_stage1_viz_gather": (_INT, [_VP, _VPP, _U64P, _U32, _U32, _F32, _U64P, _VP, _U64, _INT, _VP, _VP, _VP]),
    "cldn_hip_audit_clouds": (_INT, [_VP, _VP, _INT, _VP, _INT, _U64P, _U32, _VP, _VP, _INT]),
    "cldn_hip_audit_streams": (_INT, [_VP, _VP, _INT, _VP, _INT, _U64P, _U64P, _U32, _INT, _VP, _VP, _INT]),
    "cldn_hip_audit_last_encode": (_INT, [_VP, _VP, _VP, _INT]),
    "cldn_hip_audit_last_encode_clouds": (_I64, [_VP]),
    "cldn_hip_sweep_clouds": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _U32, _VP, _INT]),
    "cldn_hip_sweep_last_encode": (_INT, [_VP, _VP, _U32, _VP, _INT]),
    "cldn_hip_sweep_last_encode_clouds": (_I64, [_VP]),
    "cldn_hip_sweep_hist_clouds": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _U32, _VP, _INT]),
    "cldn_hip_sweep_hist_last_encode": (_INT, [_VP, _VP, _U32, _VP, _INT]),
    "cldn_hip_stream_hist": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _INT]),
    "cldn_hip_stream_hist_last_encode": (_INT, [_VP, _VP, _INT]),
    "cldn_hip_stream_crc32": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _INT]),
    "cldn_hip_stream_crc32_last_encode": (_INT, [_VP, _VP, _VP, _INT]),
    "cldn_hip_hist_entropy_bytes": (C.c_double, [_VP]),
    "cldn_hip_sweep_modes_clouds": (_INT, [_VP, _VP, _INT, _U64P, _U32, _VP, _INT]),
    "cldn_hip_sweep_modes_last_encode": (_INT, [_VP, _VP, _INT]),
    "cldn_hip_codec_set_decode_fill": (_INT, [_VP, _INT]),
    "cldn_hip_codec_set_zstd_sequences": (_INT, [_VP, _INT]),
    "cldn_hip_codec_zstd_sequences": (_INT, [_VP]),
    "cldn_hip_codec_set_zstd_matches": (_INT, [_VP, _INT]),
    "cldn_hip_codec_zstd_matches": (_INT, [_VP]),
    "cldn_hip_codec_decode_stats": (_INT, [_VP, _U32P]),
    "cldn_hip_codec_status": (_INT, [_VP]),
    "cldn_hip_codec_finish_retries": (_U32, [_VP]),
    "cldn_hip_codec_enable_timing": (_INT, [_VP, _U32]),
    "cldn_hip_codec_kernel_ms": (_INT, [_VP, _U32, _F32P]),
    "cldn_hip_codec_decode_ms": (_INT, [_VP, _F32P]),
    "cldn_hip_debug_finish_timeout_once": (_INT, [_VP]),
    "cldn_hip_debug_decode_split": (_INT, [_VP, _U32]),
    "cldn_hip_debug_zstd_seq_ring": (_U32, []),
    "cldn_hip_debug_decode_trace": (_INT, [_VP, _U32P, _U32, _U32P, _VP, _VP, _VP, _VP, _VP]),
    "cldn_hip_debug_viz_group_slots": (_INT, [_VP, _U64]),
    "cldn_hip_debug_hist_walk": (_INT, [_VP, _U32]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libcloudini_hip.so (once). Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HIP_SO):
        raise ImportError(
            f"{HIP_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(cloudini_amd has no CPU fallback)")
    # torch bundles its own HIP runtime (same SONAME, libamdhip64.so.7): whichever copy is loaded first serves the
    # whole process. When torch is going to provide device memory / streams it must be the first one in.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(HIP_SO)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc < 0:
        raise CloudiniHipError(rc, lib().cldn_hip_last_error().decode(errors="replace"))


def device_count() -> int:
    n = lib().cldn_hip_device_count()
    _check(n)
    return n


def zstd_seq_ring() -> int:
    """Test hook (cldn_hip_debug_zstd_seq_ring, a host function): the bytes of k_zstd_seq_exec's LDS ring."""
    return lib().cldn_hip_debug_zstd_seq_ring()


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _p64(a: np.ndarray):
    return a.ctypes.data_as(_U64P)


def _bytes(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _prefix(sizes) -> np.ndarray:
    """The [n + 1] uint64 prefix offsets of n sizes."""
    offs = np.zeros(len(sizes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes, dtype=np.uint64)
    return offs


def _pack(arrs: List[np.ndarray]):
    """uint8 arrays as (one buffer, its prefix offsets). One spare byte lies behind the last: an empty batch still has an address."""
    return np.concatenate(arrs + [np.zeros(1, np.uint8)]), _prefix([a.size for a in arrs])


def _pack_clouds(clouds, step: int):
    """Host clouds as (one buffer, cloud_points); refused when a cloud is no whole number of points."""
    arrs = [_bytes(c) for c in clouds]
    if any(a.size % step for a in arrs):
        raise ValueError("Input cloud_data size is not a multiple of point_step")
    return _pack(arrs)[0], np.array([a.size // step for a in arrs], dtype=np.uint64)


def _split(out: np.ndarray, offs) -> List[np.ndarray]:
    """One view of `out` per span of the prefix offsets."""
    return [out[int(offs[k]):int(offs[k + 1])] for k in range(len(offs) - 1)]


def _n_chunks(cloud_points) -> int:
    return int(sum((int(n) + 32767) // 32768 for n in cloud_points))


def _chunk_sizes(chunk_sizes, cloud_points):
    """(keep-alive array, pointer) of a decode call's `chunk_sizes`: None = the C side reads the [u32 size] prefixes."""
    if chunk_sizes is None:
        return None, None
    cs = np.ascontiguousarray(chunk_sizes, dtype=np.uint32)
    if cs.size < _n_chunks(cloud_points):  # the C side reads n_chunks sizes
        raise ValueError(f"chunk_sizes has {cs.size} entries, the batch has {_n_chunks(cloud_points)} chunks")
    return cs, _ptr(cs)


def _decode_host(codec, fn, streams, cloud_points, out, *sized) -> List[np.ndarray]:
    """A framed decode call on host buffers: fn is cldn_hip_decode_lz4 / _zstd, or cldn_hip_decode_stage1_sized with
    sized = (chunk_sizes pointer, HOST). Returns one view of `out` per cloud."""
    data, offs = _pack([_bytes(s) for s in streams])
    npts = np.array(list(cloud_points), dtype=np.uint64)
    ends = _prefix(npts * codec.plan.point_step)
    if out is None:
        out = np.zeros(max(1, int(ends[-1])), dtype=np.uint8)
    _check(fn(codec._h, _ptr(data), HOST, _p64(offs), _p64(npts), offs.size - 1, *sized, _ptr(out), int(ends[-1]), HOST))
    return _split(out, ends)


def _decode_device(codec, fn, streams_ptr, stream_offsets, cloud_points, out_ptr, out_capacity):
    """The same on device pointers, for cldn_hip_decode_lz4 / _zstd (decode_device makes its call itself)."""
    so = np.ascontiguousarray(stream_offsets, dtype=np.uint64)
    cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
    _check(fn(codec._h, C.c_void_p(streams_ptr), DEVICE, _p64(so), _p64(cp), cp.size, C.c_void_p(out_ptr), int(out_capacity),
              DEVICE))


def _decompress_host(codec, fn, spans, capacities, out):
    """cldn_hip_lz4_decompress / cldn_hip_zstd_decompress on host buffers; the return shapes of lz4_decompress_host."""
    data, bo = _pack([np.frombuffer(bytes(b), dtype=np.uint8) for b in spans])
    oo = _prefix([int(c) for c in capacities])
    n = bo.size - 1
    keep = out is not None
    if out is None:
        out = np.zeros(max(1, int(oo[-1])), dtype=np.uint8)
    sizes = np.zeros(max(1, n), dtype=np.uint32)
    rc = fn(codec._h, _ptr(data), HOST, _p64(bo), n, _ptr(out), HOST, _p64(oo), _ptr(sizes))
    if keep:
        return out, sizes[:n], rc
    _check(rc)
    return out, sizes[:n]


def _decompress_device(codec, fn, spans_ptr, span_offsets, out_ptr, out_offsets, sizes_ptr):
    bo = np.ascontiguousarray(span_offsets, dtype=np.uint64)
    oo = np.ascontiguousarray(out_offsets, dtype=np.uint64)
    _check(fn(codec._h, C.c_void_p(spans_ptr), DEVICE, _p64(bo), bo.size - 1, C.c_void_p(out_ptr), DEVICE, _p64(oo),
              C.c_void_p(sizes_ptr)))


def _report(shape, dtype) -> np.ndarray:
    rep = np.zeros(shape, dtype=dtype)
    rep.view(np.uint8)[...] = 0xEE  # (a call that fails leaves it as it was)
    return rep


def _report_arg(rep, report_ptr: int):
    """The (report pointer, location) pair of a report call: the caller's device array, else the host report."""
    return (C.c_void_p(report_ptr), DEVICE) if report_ptr else (_ptr(rep), HOST)


def _last_encode_clouds(fn, codec) -> int:
    """cldn_hip_audit_last_encode_clouds / cldn_hip_sweep_last_encode_clouds: the rows a *_last_encode report needs."""
    n = int(fn(codec._h))
    _check(n)
    return n


# cldn_hip_audit_field_t: one record per (cloud, field)
AUDIT_DTYPE = np.dtype([("n_bitwise_diff", "<u8"), ("n_class_diff", "<u8"), ("n_over_limit", "<u8"), ("first_bad_point", "<u8"),
                        ("max_abs_err", "<f8")])
AUDIT_NONE = 0xFFFFFFFFFFFFFFFF


def _limit_ptr(limit, n_fields: int):
    """(keep-alive array, pointer) of an audit call's `limit`: None = the defaults (a field's resolution, else 0)."""
    if limit is None:
        return None, None
    lim = np.ascontiguousarray(limit, dtype=np.float64)
    if lim.size != n_fields:
        raise ValueError(f"limit has {lim.size} entries, the schema has {n_fields} fields")
    return lim, lim.ctypes.data_as(C.c_void_p)


# cldn_hip_sweep_cell_t: one cell per (cloud, field, candidate resolution)
SWEEP_DTYPE = np.dtype([("bytes", "<u8"), ("n_class_diff", "<u8"), ("n_over_limit", "<u8"), ("max_abs_err", "<f8")])
SWEEP_MAX_CANDIDATES = 16


# cldn_hip_mode_cell_t: one cell per (cloud, adaptive integer field)
MODE_DTYPE = np.dtype([("bytes", "<u8", (4,)), ("probe_mode", "<u4"), ("best_mode", "<u4")])


def hist_entropy_bytes(hist) -> float:
    """cldn_hip_hist_entropy_bytes (host only): the order-0 entropy, in bytes, of the bytes a 256-bin histogram counts."""
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if h.size != 256:
        raise ValueError(f"a histogram has 256 bins, not {h.size}")
    return float(lib().cldn_hip_hist_entropy_bytes(h.ctypes.data_as(C.c_void_p)))


def _ladders(resolutions, n_fields: int) -> np.ndarray:
    """A sweep call's `resolutions` as the (n_fields, n_candidates) float32 array the C side reads."""
    res = np.ascontiguousarray(resolutions, dtype=np.float32)
    if res.ndim != 2 or res.shape[0] != n_fields:
        raise ValueError(f"resolutions must have shape (n_fields = {n_fields}, n_candidates), not {res.shape}")
    return res


class Plan:
    """cldn_hip_plan_t: the encoder/decoder selection for an EncodingInfo."""

    def __init__(self, info):
        self._h = C.c_void_p()
        arr = (_Field * max(1, len(info.fields)))()
        for i, f in enumerate(info.fields):
            arr[i].offset = int(f.offset)
            arr[i].type = int(f.type)
            arr[i].has_resolution = 0 if f.resolution is None else 1
            arr[i].resolution = 0.0 if f.resolution is None else float(f.resolution)
        _check(lib().cldn_hip_plan_create(arr, len(info.fields), int(info.point_step), int(info.version),
                                          int(info.encoding_opt), C.byref(self._h)))
        self.point_step = int(info.point_step)
        self.n_fields = len(info.fields)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.cldn_hip_plan_destroy(self._h)
            self._h = C.c_void_p()

    @property
    def uses_v5(self) -> bool:
        return bool(lib().cldn_hip_plan_uses_v5(self._h))

    @property
    def adaptive_fields(self) -> int:
        return int(lib().cldn_hip_plan_adaptive_fields(self._h))

    @property
    def max_point_bytes(self) -> int:
        return int(lib().cldn_hip_plan_max_point_bytes(self._h))

    def adaptive_field_index(self, a: int) -> int:
        """Index among the schema's fields of adaptive field a (cldn_hip_plan_adaptive_field_index)."""
        return int(lib().cldn_hip_plan_adaptive_field_index(self._h, int(a)))

    def stage1_bound(self, n_points: int) -> int:
        return int(lib().cldn_hip_stage1_bound(self._h, int(n_points)))

    def stage2_bound(self, n_points: int, stage2: int) -> int:
        return int(lib().cldn_hip_stage2_bound(self._h, int(n_points), int(stage2)))


class Codec:
    """cldn_hip_codec_t: device, stream and workspace. `stream` is a raw hipStream_t value (int) or None."""

    def __init__(self, plan: Plan, device: int = -1, stream: Optional[int] = None):
        self.plan = plan
        self._h = C.c_void_p()
        _check(lib().cldn_hip_codec_create(plan._h, device, C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.cldn_hip_codec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()

    def synchronize(self):
        _check(lib().cldn_hip_codec_synchronize(self._h))

    def status(self):
        _check(lib().cldn_hip_codec_status(self._h))

    def stream(self) -> int:
        """cldn_hip_codec_stream: the raw hipStream_t the codec enqueues on (the caller's, or the one it created), as an
        int -- e.g. for torch.cuda.ExternalStream."""
        return int(lib().cldn_hip_codec_stream(self._h) or 0)

    def viz_preprocess_host(self, cloud, point_step: int, xyz_offset: int, resolution: float) -> np.ndarray:
        """applyVizLossyPreprocessing's data path on host buffers: the surviving points, order preserved."""
        data = _bytes(cloud)
        out = np.empty(max(1, data.size), dtype=np.uint8)
        kept = C.c_uint64(0)
        _check(lib().cldn_hip_viz_preprocess(self._h, _ptr(data), HOST, data.size // point_step, point_step, xyz_offset,
                                             resolution, _ptr(out), out.size, HOST, C.byref(kept)))
        return out[: kept.value * point_step].copy()

    def viz_preprocess_device(self, points_ptr: int, n_points: int, point_step: int, xyz_offset: int, resolution: float,
                              out_ptr: int, out_capacity: int) -> int:
        kept = C.c_uint64(0)
        _check(lib().cldn_hip_viz_preprocess(self._h, C.c_void_p(points_ptr), DEVICE, n_points, point_step, xyz_offset,
                                             resolution, C.c_void_p(out_ptr), out_capacity, DEVICE, C.byref(kept)))
        return int(kept.value)

    def viz_group_slots(self, slots: int):
        """Test hook (cldn_hip_debug_viz_group_slots): table slots per cloud group of the batched pre-filter, 0 = default."""
        _check(lib().cldn_hip_debug_viz_group_slots(self._h, int(slots)))

    def viz_preprocess_batch_host(self, clouds: Sequence[np.ndarray], point_step: int, xyz_offset: int, resolution: float,
                                  guard: int = 0):
        """cldn_hip_viz_preprocess_batch on host buffers. Returns (survivors per cloud, kept_points, tail): `tail` is the output
        buffer behind the last survivor, `guard` bytes of it beyond the capacity handed to the call (filled with 0xA5)."""
        arrs = [_bytes(c) for c in clouds]
        npts = np.array([a.size // point_step for a in arrs], dtype=np.uint64)
        data, _ = _pack(arrs)
        cap = int(npts.sum()) * point_step
        out = np.full(cap + guard + 1, 0xA5, dtype=np.uint8)
        kept = np.zeros(max(1, len(arrs)), dtype=np.uint64)
        _check(lib().cldn_hip_viz_preprocess_batch(self._h, _ptr(data), HOST, _p64(npts), len(arrs), point_step, xyz_offset,
                                                   resolution, _ptr(out), cap, HOST, _p64(kept)))
        kept = kept[: len(arrs)]
        ends = _prefix(kept * int(point_step))
        return [v.copy() for v in _split(out, ends)], kept, out[int(ends[-1]):cap + guard]

    def viz_preprocess_batch_device(self, points_ptr: int, cloud_points, point_step: int, xyz_offset: int, resolution: float,
                                    out_ptr: int, out_capacity: int) -> np.ndarray:
        """The same on device buffers; returns kept_points (the call has synchronised)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        kept = np.zeros(max(1, cp.size), dtype=np.uint64)
        _check(lib().cldn_hip_viz_preprocess_batch(self._h, C.c_void_p(points_ptr), DEVICE, _p64(cp), cp.size, point_step, xyz_offset,
                                                   resolution, C.c_void_p(out_ptr), int(out_capacity), DEVICE, _p64(kept)))
        return kept[: cp.size]

    def encode_viz(self, clouds: Sequence[np.ndarray], xyz_offset: int, resolution: float, gather: bool = False,
                   two_step: bool = False):
        """cldn_hip_encode_stage1_viz (or _gather: one host buffer per cloud) with host outputs, sized by the INPUT counts;
        two_step: out = NULL, then cldn_hip_codec_fetch_output. Returns (streams, chunk_sizes, modes, kept_points) of the
        filtered clouds, shaped like encode_host's."""
        step = self.plan.point_step
        arrs = [_bytes(c) for c in clouds]
        npts = np.array([a.size // step for a in arrs], dtype=np.uint64)
        n = len(arrs)
        cap = self._out_capacity(npts)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        chunk_sizes = np.zeros(max(1, _n_chunks(npts)), dtype=np.uint32)
        na = self.plan.adaptive_fields
        modes = np.full(max(1, n * max(1, na)), 0xEE, dtype=np.uint8)
        kept = np.zeros(max(1, n), dtype=np.uint64)
        tail = (None if two_step else _ptr(out), 0 if two_step else cap, HOST, _ptr(offs), _ptr(chunk_sizes), _ptr(modes))
        if gather:
            ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data if a.size else None for a in arrs])
            _check(lib().cldn_hip_encode_stage1_viz_gather(self._h, ptrs, _p64(npts), n, xyz_offset, resolution, _p64(kept), *tail))
        else:
            data, _ = _pack(arrs)
            _check(lib().cldn_hip_encode_stage1_viz(self._h, _ptr(data), HOST, _p64(npts), n, xyz_offset, resolution, _p64(kept),
                                                    *tail))
        if two_step:
            _check(lib().cldn_hip_codec_fetch_output(self._h, _ptr(out), int(offs[n])))
        kept = kept[:n]
        streams = [v.copy() for v in _split(out, offs)]
        return streams, chunk_sizes[:_n_chunks(kept)].copy(), modes[: n * na].reshape(n, na).copy(), kept

    def encode_viz_device(self, points_ptr: int, cloud_points, xyz_offset: int, resolution: float, out_ptr: int,
                          out_capacity: int, stream_offsets_ptr: int = 0, chunk_sizes_ptr: int = 0, modes_ptr: int = 0):
        """cldn_hip_encode_stage1_viz on device-resident points with device outputs; returns kept_points."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        kept = np.zeros(max(1, cp.size), dtype=np.uint64)
        _check(lib().cldn_hip_encode_stage1_viz(
            self._h, C.c_void_p(points_ptr), DEVICE, _p64(cp), cp.size, xyz_offset, resolution, _p64(kept), C.c_void_p(out_ptr),
            int(out_capacity), DEVICE, C.c_void_p(stream_offsets_ptr), C.c_void_p(chunk_sizes_ptr), C.c_void_p(modes_ptr)))
        return kept[: cp.size]

    def set_zstd_sequences(self, on: bool):
        """cldn_hip_codec_set_zstd_sequences: True = the ZSTD read side takes frames with sequences (default off: they are
        handed to the host). See include/cloudini_hip.h for what it costs."""
        _check(lib().cldn_hip_codec_set_zstd_sequences(self._h, 1 if on else 0))

    def zstd_sequences(self) -> bool:
        return bool(lib().cldn_hip_codec_zstd_sequences(self._h))

    def set_zstd_matches(self, on: bool):
        """cldn_hip_codec_set_zstd_matches: True = the ZSTD writer (set_stage2(STAGE2_ZSTD)) turns matches of the device's match
        search into sequences (default off: literal-only blocks). See include/cloudini_hip.h for when it pays."""
        _check(lib().cldn_hip_codec_set_zstd_matches(self._h, 1 if on else 0))

    def zstd_matches(self) -> bool:
        return bool(lib().cldn_hip_codec_zstd_matches(self._h))

    def set_decode_fill(self, zero: bool):
        """cldn_hip_codec_set_decode_fill: True = bytes no field covers may be written as 0 (no round trip of a host buffer)."""
        _check(lib().cldn_hip_codec_set_decode_fill(self._h, 1 if zero else 0))

    def decode_stats(self):
        """Chunks of the last decode call per kernel: (fast regular, fast sections, serial chunks, serial sections)."""
        v = (C.c_uint32 * 4)()
        _check(lib().cldn_hip_codec_decode_stats(self._h, v))
        return tuple(int(x) for x in v)

    def decode_trace(self, max_chunks: int = 4096):
        """Test hook (cldn_hip_debug_decode_trace): what the last decode call decided, after a stream synchronise. Returns a dict:
        `words` = status words 8..15 (fast regular, fast sections, serial chunks, serial sections, folded by the Palette guess,
        k_section_dv_w chunks, sections with mode byte 0, DeltaVarint guesses from the end) and per chunk reg_end_pre,
        slices_done, sec_cols, reg_end, sec_done."""
        words = (C.c_uint32 * 8)()
        n = C.c_uint32(0)
        u32 = [np.zeros(max(1, max_chunks), dtype=np.uint32) for _ in range(3)]
        u8 = [np.zeros(max(1, max_chunks), dtype=np.uint8) for _ in range(2)]
        _check(lib().cldn_hip_debug_decode_trace(self._h, words, max_chunks, C.byref(n), _ptr(u32[0]), _ptr(u32[1]), _ptr(u8[0]),
                                                 _ptr(u32[2]), _ptr(u8[1])))
        k = int(n.value)
        return {"words": tuple(int(x) for x in words), "n_chunks": k, "reg_end_pre": u32[0][:k].copy(),
                "slices_done": u32[1][:k].copy(), "sec_cols": u8[0][:k].copy(), "reg_end": u32[2][:k].copy(),
                "sec_done": u8[1][:k].copy()}

    def finish_retries(self) -> int:
        """Calls redone through k_finish's ticket order after ST_FINISH_TIMEOUT (cldn_hip_codec_finish_retries)."""
        return int(lib().cldn_hip_codec_finish_retries(self._h))

    def finish_timeout_once(self) -> int:
        """Test hook (cldn_hip_debug_finish_timeout_once): the next encode call reports ST_FINISH_TIMEOUT on its first attempt.
        Returns the C return code."""
        return lib().cldn_hip_debug_finish_timeout_once(self._h)

    def decode_split(self, parts: int) -> int:
        """Test hook (cldn_hip_debug_decode_split): the point decoder's launch shape -- 0 = by the number of chunks (default),
        1 = the chained launch, 2..16 = a SPLIT launch with that many workgroups per chunk. Returns the C return code."""
        return lib().cldn_hip_debug_decode_split(self._h, int(parts))

    def force_modes(self, modes=None):
        """Adaptive-int modes committed elsewhere (cldn_hip_codec_force_modes); None / empty returns to probing."""
        if modes is None or len(modes) == 0:
            _check(lib().cldn_hip_codec_force_modes(self._h, None, 0))
            return
        m = np.ascontiguousarray(modes, dtype=np.uint8)
        _check(lib().cldn_hip_codec_force_modes(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.size))

    def force_modes_per_cloud(self, modes=None):
        """One mode set per cloud of the following encode calls (cldn_hip_codec_force_modes_per_cloud): modes has shape
        (n_clouds, adaptive fields), e.g. the best_mode column of sweep_modes_*; None / empty returns to probing. The streams
        are then valid Cloudini streams, but not the reference encoder's bytes."""
        if modes is None or len(modes) == 0:
            _check(lib().cldn_hip_codec_force_modes_per_cloud(self._h, None, 0))
            return
        m = np.ascontiguousarray(modes, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.plan.adaptive_fields:
            raise ValueError(f"modes must have shape (n_clouds, adaptive fields = {self.plan.adaptive_fields}), not {m.shape}")
        _check(lib().cldn_hip_codec_force_modes_per_cloud(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.shape[0]))

    def set_stage2(self, stage2: int):
        """0 = stage-1 streams (default), 1 = [u32 size][LZ4 block] per chunk, compressed on the device, 2 = the same with the
        FAST parameters (4 KiB sub-ranges: ~1.5 x the speed, blocks ~3 % larger), 3 (STAGE2_ZSTD) = [u32 size][ZSTD frame of
        literal-only blocks] per chunk: valid frames for any ZSTD decoder, not libzstd's bytes."""
        _check(lib().cldn_hip_codec_set_stage2(self._h, int(stage2)))
        self._stage2 = int(stage2)

    def pipeline(self, mode: int = 0, points_ptr: int = 0) -> int:
        """Choose the encoder pipeline (cldn_hip_codec_pipeline: 0 auto, 1 generic kernel + slots, 2 piece kernel + slots);
        returns the pipeline the next call takes."""
        r = lib().cldn_hip_codec_pipeline(self._h, int(mode), C.c_void_p(points_ptr))
        _check(r)
        return int(r)

    def enable_timing(self, n_slots: int):
        _check(lib().cldn_hip_codec_enable_timing(self._h, int(n_slots)))

    def kernel_ms(self, slot: int):
        v = (C.c_float * 4)()
        _check(lib().cldn_hip_codec_kernel_ms(self._h, int(slot), v))
        return {"regular": v[0], "sections": v[1], "compact": v[2], "total": v[3]}

    def decode_ms(self):
        """HIP-event times of the last decode call (timing enabled): the regular-stream kernel, everything launched."""
        v = (C.c_float * 2)()
        _check(lib().cldn_hip_codec_decode_ms(self._h, v))
        return {"regular_kernel": v[0], "total": v[1]}

    # ---- host buffers (numpy) -------------------------------------------------------------------------
    def encode_host(self, clouds: Sequence[np.ndarray]):
        """Encode a batch of host-resident clouds. Returns (list of framed stage-1 streams, chunk_sizes, modes)."""
        data, npts = _pack_clouds(clouds, self.plan.point_step)
        n = npts.size
        cap = self._out_capacity(npts)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        chunk_sizes = np.zeros(max(1, _n_chunks(npts)), dtype=np.uint32)
        na = self.plan.adaptive_fields
        modes = np.zeros(max(1, n * max(1, na)), dtype=np.uint8)
        _check(lib().cldn_hip_encode_stage1(self._h, _ptr(data), HOST, _p64(npts), n, _ptr(out), cap, HOST, _ptr(offs),
                                            _ptr(chunk_sizes), _ptr(modes)))
        streams = [v.copy() for v in _split(out, offs)]
        return streams, chunk_sizes[:_n_chunks(npts)], modes[: n * na].reshape(n, na)

    def _out_capacity(self, cloud_points) -> int:
        """Bytes that the streams of a batch can take under the codec's stage 2."""
        return int(sum(self.plan.stage2_bound(int(n), getattr(self, "_stage2", 0)) for n in cloud_points))

    # ---- chunk-table output ----------------------------------------------------------------------------
    def encode_chunks_device(self, points_ptr: int, cloud_points: np.ndarray, modes_ptr: int = 0) -> ChunkTable:
        """cldn_hip_encode_stage1_chunks on device-resident points: stage 1 without the framing (asynchronous)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        table = ChunkTable()
        _check(lib().cldn_hip_encode_stage1_chunks(self._h, C.c_void_p(points_ptr), DEVICE, cp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   cp.size, C.byref(table), C.c_void_p(modes_ptr)))
        return table

    def frame_chunks_device(self, out_ptr: int, out_capacity: int, stream_offsets_ptr: int = 0, chunk_sizes_ptr: int = 0):
        _check(lib().cldn_hip_frame_chunks(self._h, C.c_void_p(out_ptr), int(out_capacity), DEVICE, C.c_void_p(stream_offsets_ptr),
                                           C.c_void_p(chunk_sizes_ptr)))

    # ---- device buffers (raw pointers, e.g. torch tensors' data_ptr()) ---------------------------------
    def encode_device(self, points_ptr: int, cloud_points: np.ndarray, out_ptr: int, out_capacity: int,
                      stream_offsets_ptr: int = 0, chunk_sizes_ptr: int = 0, modes_ptr: int = 0):
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        _check(lib().cldn_hip_encode_stage1(
            self._h, C.c_void_p(points_ptr), DEVICE, cp.ctypes.data_as(C.POINTER(C.c_uint64)), cp.size,
            C.c_void_p(out_ptr), int(out_capacity), DEVICE, C.c_void_p(stream_offsets_ptr),
            C.c_void_p(chunk_sizes_ptr), C.c_void_p(modes_ptr)))

    def decode_host(self, streams: Sequence[np.ndarray], cloud_points: Sequence[int],
                    out: Optional[np.ndarray] = None, chunk_sizes=None) -> List[np.ndarray]:
        cloud_points = list(cloud_points)
        cs, cs_ptr = _chunk_sizes(chunk_sizes, cloud_points)
        return _decode_host(self, lib().cldn_hip_decode_stage1_sized, streams, cloud_points, out, cs_ptr, HOST)

    def decode_device(self, streams_ptr: int, stream_offsets: np.ndarray, cloud_points: np.ndarray, out_ptr: int,
                      out_capacity: int, chunk_sizes_ptr: int = 0):
        """chunk_sizes_ptr: device array of the chunks' payload sizes (what encode_device reported): the chunk table is then
        built in parallel (cldn_hip_decode_stage1_sized)."""
        so = np.ascontiguousarray(stream_offsets, dtype=np.uint64)
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        _check(lib().cldn_hip_decode_stage1_sized(
            self._h, C.c_void_p(streams_ptr), DEVICE, so.ctypes.data_as(C.POINTER(C.c_uint64)),
            cp.ctypes.data_as(C.POINTER(C.c_uint64)), cp.size, C.c_void_p(chunk_sizes_ptr), DEVICE, C.c_void_p(out_ptr),
            int(out_capacity), DEVICE))

    def decode_unframed_device(self, payload_ptr: int, size: int, out_ptr: int, out_capacity: int):
        """cldn_hip_decode_stage1_unframed on device buffers (wire version 2: one run of points without [u32 size] prefixes,
        decoded until it is empty). Asynchronous: a payload that holds more points than out_capacity shows in status()."""
        _check(lib().cldn_hip_decode_stage1_unframed(self._h, C.c_void_p(payload_ptr), int(size), DEVICE, C.c_void_p(out_ptr),
                                                     int(out_capacity), DEVICE))

    # ---- LZ4 blocks back into bytes (cldn_hip_lz4_decompress / cldn_hip_decode_lz4) --------------------------------
    def lz4_decompress_host(self, blocks: Sequence[bytes], capacities: Sequence[int], out: Optional[np.ndarray] = None):
        """A batch of LZ4 blocks from host memory; block k may decode to capacities[k] bytes. Returns (out, sizes): the spans
        back to back in `out` (span k starts at sum(capacities[:k])), sizes[k] = decoded bytes or 0xffffffff for a refused
        block. Raises CloudiniHipError (CORRUPT) when a block is refused unless `out` is given -- then the error is returned
        as a third element so that the caller can look at the other blocks."""
        return _decompress_host(self, lib().cldn_hip_lz4_decompress, blocks, capacities, out)

    def lz4_decompress_device(self, blocks_ptr: int, block_offsets: np.ndarray, out_ptr: int, out_offsets: np.ndarray,
                              sizes_ptr: int):
        """The same on device buffers (asynchronous; refused blocks show in sizes and in status())."""
        _decompress_device(self, lib().cldn_hip_lz4_decompress, blocks_ptr, block_offsets, out_ptr, out_offsets, sizes_ptr)

    def decode_lz4_host(self, streams: Sequence[np.ndarray], cloud_points: Sequence[int],
                        out: Optional[np.ndarray] = None) -> List[np.ndarray]:
        """decode_host for streams whose chunks are [u32 block size][LZ4 block] (the body of an LZ4 message)."""
        return _decode_host(self, lib().cldn_hip_decode_lz4, streams, cloud_points, out)

    def decode_lz4_device(self, streams_ptr: int, stream_offsets: np.ndarray, cloud_points: np.ndarray, out_ptr: int,
                          out_capacity: int):
        _decode_device(self, lib().cldn_hip_decode_lz4, streams_ptr, stream_offsets, cloud_points, out_ptr, out_capacity)

    # ---- ZSTD frames without sequences back into bytes (cldn_hip_zstd_decompress / cldn_hip_decode_zstd) ----------
    def zstd_decompress_host(self, frames: Sequence[bytes], capacities: Sequence[int], out: Optional[np.ndarray] = None):
        """A batch of ZSTD frames from host memory; frame k may decode to capacities[k] bytes. Returns (out, sizes): the spans
        back to back in `out` (span k starts at sum(capacities[:k])), sizes[k] = decoded bytes, 0xffffffff for a refused
        frame, 0xfffffffe for one that needs the host (sequences, checksum, ...). Raises CloudiniHipError (CORRUPT, else
        UNSUPPORTED) for those unless `out` is given -- then the error is returned as a third element so that the caller
        can look at the other frames."""
        return _decompress_host(self, lib().cldn_hip_zstd_decompress, frames, capacities, out)

    def zstd_decompress_device(self, frames_ptr: int, frame_offsets: np.ndarray, out_ptr: int, out_offsets: np.ndarray,
                              sizes_ptr: int):
        """The same on device buffers (asynchronous; the verdicts show in sizes and in status())."""
        _decompress_device(self, lib().cldn_hip_zstd_decompress, frames_ptr, frame_offsets, out_ptr, out_offsets, sizes_ptr)

    def decode_zstd_host(self, streams: Sequence[np.ndarray], cloud_points: Sequence[int],
                        out: Optional[np.ndarray] = None) -> List[np.ndarray]:
        """decode_host for streams whose chunks are [u32 frame size][ZSTD frame] (the body of a ZSTD message); UNSUPPORTED
        when a frame carries sequences or options the device decoder does not take."""
        return _decode_host(self, lib().cldn_hip_decode_zstd, streams, cloud_points, out)

    def decode_zstd_device(self, streams_ptr: int, stream_offsets: np.ndarray, cloud_points: np.ndarray, out_ptr: int,
                          out_capacity: int):
        _decode_device(self, lib().cldn_hip_decode_zstd, streams_ptr, stream_offsets, cloud_points, out_ptr, out_capacity)

    # ---- LZ4 / ZSTD message bodies where they lie (cldn_hip_decode_lz4_gather / cldn_hip_decode_zstd_gather) ---------
    def decode_stage2_gather(self, stage2: int, bodies: Sequence[np.ndarray], cloud_points: Sequence[int], chunk_sizes=None,
                             expanded=None, out: Optional[np.ndarray] = None):
        """stage2: STAGE2_LZ4 or STAGE2_ZSTD. bodies: one uint8 array per message, read at the address it has (a view at any
        offset of a larger array is taken as it is). chunk_sizes: the [u32 size] prefixes, or None. expanded: None, or one
        entry per chunk of the batch -- None or the chunk's stage-1 payload (uint8 array / bytes). Returns (clouds, verdicts,
        rc): the decoded clouds (views of `out`), the per-chunk verdicts, the call's return code (0 = OK; the error text is
        cldn_hip_last_error's)."""
        step = self.plan.point_step
        arrs = [b if isinstance(b, np.ndarray) and b.dtype == np.uint8 and b.ndim == 1 and b.strides[0] == 1
                else np.frombuffer(bytes(b), dtype=np.uint8) for b in bodies]
        n = len(arrs)
        ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data if a.size else None for a in arrs])
        sizes = np.array([a.size for a in arrs], dtype=np.uint64)
        npts = np.array(list(cloud_points), dtype=np.uint64)
        n_chunks = _n_chunks(npts)
        ends = _prefix(npts * step)
        total = int(ends[-1])
        if out is None:
            out = np.zeros(max(1, total), dtype=np.uint8)
        cs, cs_ptr = _chunk_sizes(chunk_sizes, npts)
        verdicts = np.full(max(1, n_chunks), 0xEEEEEEEE, dtype=np.uint32)
        exp_ptrs = exp_sizes = None
        keep = []
        if expanded is not None:
            if len(expanded) != n_chunks:
                raise ValueError(f"expanded has {len(expanded)} entries, the batch has {n_chunks} chunks")
            # (one spare byte behind every payload: an empty one still has an address)
            keep = [None if e is None else np.frombuffer(bytes(e) + b"\0", dtype=np.uint8)[:len(bytes(e))] for e in expanded]
            exp_ptrs = (C.c_void_p * max(1, n_chunks))(*[None if e is None else e.ctypes.data for e in keep])
            exp_sizes = np.array([0 if e is None else e.size for e in keep], dtype=np.uint32)
        fn = lib().cldn_hip_decode_lz4_gather if stage2 == STAGE2_LZ4 else lib().cldn_hip_decode_zstd_gather
        rc = fn(self._h, ptrs, _p64(sizes), _p64(npts), n, cs_ptr, exp_ptrs, None if exp_sizes is None else _ptr(exp_sizes),
                _ptr(verdicts), _ptr(out), total, HOST)
        return _split(out, ends), verdicts[:n_chunks], rc

    # ---- audit: per-field error reports (cldn_hip_audit_*) -----------------------------------------------------------
    def audit_clouds_host(self, a: Sequence[np.ndarray], b: Sequence[np.ndarray], limit=None, report: Optional[np.ndarray] = None):
        """cldn_hip_audit_clouds on host buffers: clouds a[k] against b[k]. Returns the (n_clouds, n_fields) report."""
        step = self.plan.point_step
        aa, bb = [_bytes(x) for x in a], [_bytes(x) for x in b]
        if [x.size for x in aa] != [x.size for x in bb] or any(x.size % step for x in aa):
            raise ValueError("the two batches must have the same whole number of points per cloud")
        cp = np.array([x.size // step for x in aa], dtype=np.uint64)
        (da, _), (db, _) = _pack(aa), _pack(bb)
        rep = _report((len(aa), self.plan.n_fields), AUDIT_DTYPE) if report is None else report
        lim, lp = _limit_ptr(limit, self.plan.n_fields)
        _check(lib().cldn_hip_audit_clouds(self._h, _ptr(da), HOST, _ptr(db), HOST, _p64(cp), cp.size, lp, _ptr(rep), HOST))
        return rep

    def audit_clouds_device(self, a_ptr: int, b_ptr: int, cloud_points, limit=None, report_ptr: int = 0, a_loc: int = DEVICE,
                            b_loc: int = DEVICE):
        """cldn_hip_audit_clouds on raw pointers. report_ptr: device array of n_clouds * n_fields records (the call only
        enqueues work when both buffers are on the device; returns None), 0 = host report (returned)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        lim, lp = _limit_ptr(limit, self.plan.n_fields)
        rep = None if report_ptr else _report((cp.size, self.plan.n_fields), AUDIT_DTYPE)
        _check(lib().cldn_hip_audit_clouds(self._h, C.c_void_p(a_ptr), a_loc, C.c_void_p(b_ptr), b_loc, _p64(cp), cp.size, lp,
                                           *_report_arg(rep, report_ptr)))
        return rep

    def audit_streams_host(self, clouds: Sequence[np.ndarray], streams: Sequence[np.ndarray], stream_kind: int = 0, limit=None,
                           report: Optional[np.ndarray] = None):
        """cldn_hip_audit_streams on host buffers: clouds[k] against the decode of streams[k] (stream_kind 0: framed stage-1
        streams, 1: [u32 size][LZ4 block] per chunk)."""
        pts = [_bytes(x) for x in clouds]
        cp = np.array([x.size // self.plan.point_step for x in pts], dtype=np.uint64)
        (dp, _), (ds, offs) = _pack(pts), _pack([_bytes(x) for x in streams])
        rep = _report((len(pts), self.plan.n_fields), AUDIT_DTYPE) if report is None else report
        lim, lp = _limit_ptr(limit, self.plan.n_fields)
        _check(lib().cldn_hip_audit_streams(self._h, _ptr(dp), HOST, _ptr(ds), HOST, _p64(offs), _p64(cp), cp.size, int(stream_kind),
                                            lp, _ptr(rep), HOST))
        return rep

    def audit_streams_device(self, points_ptr: int, streams_ptr: int, stream_offsets, cloud_points, stream_kind: int = 0,
                             limit=None, report_ptr: int = 0):
        """The same on device buffers; report_ptr as in audit_clouds_device."""
        so = np.ascontiguousarray(stream_offsets, dtype=np.uint64)
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        lim, lp = _limit_ptr(limit, self.plan.n_fields)
        rep = None if report_ptr else _report((cp.size, self.plan.n_fields), AUDIT_DTYPE)
        _check(lib().cldn_hip_audit_streams(self._h, C.c_void_p(points_ptr), DEVICE, C.c_void_p(streams_ptr), DEVICE, _p64(so),
                                            _p64(cp), cp.size, int(stream_kind), lp, *_report_arg(rep, report_ptr)))
        return rep

    def audit_last_encode(self, limit=None, report_ptr: int = 0):
        """cldn_hip_audit_last_encode: this codec's most recent encode call against the decode of what it wrote; one row per
        cloud of that call (the filtered clouds of a viz call). Raises CloudiniHipError (ARG) when another call came between."""
        n = _last_encode_clouds(lib().cldn_hip_audit_last_encode_clouds, self)
        lim, lp = _limit_ptr(limit, self.plan.n_fields)
        rep = None if report_ptr else _report((n, self.plan.n_fields), AUDIT_DTYPE)
        _check(lib().cldn_hip_audit_last_encode(self._h, lp, *_report_arg(rep, report_ptr)))
        return rep

    # ---- resolution sweep: size and error per field and candidate (cldn_hip_sweep_*) ---------------------------------
    def sweep_clouds_host(self, clouds: Sequence[np.ndarray], resolutions) -> np.ndarray:
        """cldn_hip_sweep_clouds on host buffers. resolutions: (n_fields, n_candidates), one ladder per field, 0 = skip.
        Returns the (n_clouds, n_fields, n_candidates) report."""
        data, cp = _pack_clouds(clouds, self.plan.point_step)
        return self.sweep_clouds_device(data.ctypes.data, cp, resolutions, points_loc=HOST)

    def sweep_clouds_device(self, points_ptr: int, cloud_points, resolutions, report_ptr: int = 0, points_loc: int = DEVICE):
        """cldn_hip_sweep_clouds on a raw pointer. report_ptr: device array of n_clouds * n_fields * n_candidates cells (the call
        only enqueues work when the points are on the device; returns None), 0 = host report (returned)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        res = _ladders(resolutions, self.plan.n_fields)
        rep = None if report_ptr else _report((cp.size, self.plan.n_fields, res.shape[1]), SWEEP_DTYPE)
        _check(lib().cldn_hip_sweep_clouds(self._h, C.c_void_p(points_ptr), points_loc, _p64(cp), cp.size, _ptr(res), res.shape[1],
                                           *_report_arg(rep, report_ptr)))
        return rep

    def sweep_last_encode(self, resolutions, report_ptr: int = 0):
        """cldn_hip_sweep_last_encode: the points of this codec's most recent encode call (the survivors of a viz call), one row
        per cloud of that call. Valid from the encode call on (a chunk table need not be framed); leaves the state for
        audit_last_encode as it found it. Raises CloudiniHipError (ARG) when another call came between."""
        n = _last_encode_clouds(lib().cldn_hip_sweep_last_encode_clouds, self)
        res = _ladders(resolutions, self.plan.n_fields)
        rep = None if report_ptr else _report((n, self.plan.n_fields, res.shape[1]), SWEEP_DTYPE)
        _check(lib().cldn_hip_sweep_last_encode(self._h, _ptr(res), res.shape[1], *_report_arg(rep, report_ptr)))
        return rep

    # ---- byte histograms for the stage-2 estimate (cldn_hip_sweep_hist_*, cldn_hip_stream_hist*) ---------------------
    def hist_walk(self, blocks: int):
        """Test and measurement hook (cldn_hip_debug_hist_walk): 1024-point blocks per workgroup of k_sweep_hist, 0 = default."""
        _check(lib().cldn_hip_debug_hist_walk(self._h, int(blocks)))

    def sweep_hist_clouds_host(self, clouds: Sequence[np.ndarray], resolutions) -> np.ndarray:
        """cldn_hip_sweep_hist_clouds on host buffers; arguments as sweep_clouds_host. Returns the
        (n_clouds, n_fields, n_candidates, 256) uint64 report."""
        data, cp = _pack_clouds(clouds, self.plan.point_step)
        return self.sweep_hist_clouds_device(data.ctypes.data, cp, resolutions, points_loc=HOST)

    def sweep_hist_clouds_device(self, points_ptr: int, cloud_points, resolutions, report_ptr: int = 0, points_loc: int = DEVICE):
        """cldn_hip_sweep_hist_clouds on a raw pointer; report_ptr as in sweep_clouds_device (2048 bytes per histogram)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        res = _ladders(resolutions, self.plan.n_fields)
        rep = None if report_ptr else _report((cp.size, self.plan.n_fields, res.shape[1], 256), np.uint64)
        _check(lib().cldn_hip_sweep_hist_clouds(self._h, C.c_void_p(points_ptr), points_loc, _p64(cp), cp.size, _ptr(res),
                                                res.shape[1], *_report_arg(rep, report_ptr)))
        return rep

    def sweep_hist_last_encode(self, resolutions, report_ptr: int = 0):
        """cldn_hip_sweep_hist_last_encode: the points of this codec's most recent encode call; state rules as sweep_last_encode."""
        n = _last_encode_clouds(lib().cldn_hip_sweep_last_encode_clouds, self)
        res = _ladders(resolutions, self.plan.n_fields)
        rep = None if report_ptr else _report((n, self.plan.n_fields, res.shape[1], 256), np.uint64)
        _check(lib().cldn_hip_sweep_hist_last_encode(self._h, _ptr(res), res.shape[1], *_report_arg(rep, report_ptr)))
        return rep

    def stream_hist_host(self, streams: Sequence[np.ndarray]) -> np.ndarray:
        """cldn_hip_stream_hist on host buffers: one (256,) uint64 histogram per stream."""
        data, offs = _pack([_bytes(x) for x in streams])
        return self.stream_hist_device(data.ctypes.data, offs, streams_loc=HOST)

    def stream_hist_device(self, streams_ptr: int, stream_offsets, report_ptr: int = 0, streams_loc: int = DEVICE):
        """cldn_hip_stream_hist on a raw pointer. stream_offsets: host [n_clouds + 1]; report_ptr: device array of n_clouds
        histograms (returns None), 0 = host report (returned)."""
        so = np.ascontiguousarray(stream_offsets, dtype=np.uint64)
        n = max(0, so.size - 1)
        rep = None if report_ptr else _report((n, 256), np.uint64)
        _check(lib().cldn_hip_stream_hist(self._h, C.c_void_p(streams_ptr), streams_loc, _p64(so), n, *_report_arg(rep, report_ptr)))
        return rep

    def stream_hist_last_encode(self, report_ptr: int = 0):
        """cldn_hip_stream_hist_last_encode: the streams this codec's most recent framed encode call wrote, one row per cloud."""
        n = _last_encode_clouds(lib().cldn_hip_audit_last_encode_clouds, self)
        rep = None if report_ptr else _report((n, 256), np.uint64)
        _check(lib().cldn_hip_stream_hist_last_encode(self._h, *_report_arg(rep, report_ptr)))
        return rep

    # ---- CRC-32 of byte spans (cldn_hip_stream_crc32*) --------------------------------------------------------------
    def stream_crc32_host(self, streams: Sequence[np.ndarray]) -> np.ndarray:
        """cldn_hip_stream_crc32 on host buffers: zlib.crc32 of each stream, a (n,) uint32 array."""
        data, offs = _pack([_bytes(x) for x in streams])
        return self.stream_crc32_device(data.ctypes.data, offs, streams_loc=HOST)

    def stream_crc32_device(self, streams_ptr: int, stream_offsets, crc_ptr: int = 0, streams_loc: int = DEVICE):
        """cldn_hip_stream_crc32 on a raw pointer. stream_offsets: host [n + 1]; crc_ptr: device array of n uint32 (returns
        None), 0 = host result (returned)."""
        so = np.ascontiguousarray(stream_offsets, dtype=np.uint64)
        n = max(0, so.size - 1)
        crc = None if crc_ptr else _report((n,), np.uint32)
        _check(lib().cldn_hip_stream_crc32(self._h, C.c_void_p(streams_ptr), streams_loc, _p64(so), n, *_report_arg(crc, crc_ptr)))
        return crc

    def stream_crc32_last_encode(self, crc_ptr: int = 0, sizes_ptr: int = 0):
        """cldn_hip_stream_crc32_last_encode: CRC-32 and length of the framed stage-1 stream of each cloud of this codec's most
        recent framed encode call, whatever its stage 2. Returns (crc uint32 [n], sizes uint64 [n]) on the host, or None when
        crc_ptr names a device array (sizes_ptr: a device array as well, or 0 for none)."""
        n = _last_encode_clouds(lib().cldn_hip_audit_last_encode_clouds, self)
        if crc_ptr:
            _check(lib().cldn_hip_stream_crc32_last_encode(self._h, C.c_void_p(crc_ptr), C.c_void_p(sizes_ptr), DEVICE))
            return None
        crc, sizes = _report((n,), np.uint32), _report((n,), np.uint64)
        _check(lib().cldn_hip_stream_crc32_last_encode(self._h, _ptr(crc), _ptr(sizes), HOST))
        return crc, sizes

    # ---- adaptive integer modes: section bytes per mode, probed and best mode (cldn_hip_sweep_modes_*) ---------------
    def sweep_modes_host(self, clouds: Sequence[np.ndarray]) -> np.ndarray:
        """cldn_hip_sweep_modes_clouds on host buffers. Returns the (n_clouds, adaptive fields) report."""
        data, cp = _pack_clouds(clouds, self.plan.point_step)
        return self.sweep_modes_device(data.ctypes.data, cp, points_loc=HOST)

    def sweep_modes_device(self, points_ptr: int, cloud_points, report_ptr: int = 0, points_loc: int = DEVICE):
        """cldn_hip_sweep_modes_clouds on a raw pointer. report_ptr: device array of n_clouds * adaptive fields cells (the call
        only enqueues work when the points are on the device; returns None), 0 = host report (returned)."""
        cp = np.ascontiguousarray(cloud_points, dtype=np.uint64)
        rep = None if report_ptr else _report((cp.size, self.plan.adaptive_fields), MODE_DTYPE)
        _check(lib().cldn_hip_sweep_modes_clouds(self._h, C.c_void_p(points_ptr), points_loc, _p64(cp), cp.size,
                                                 *_report_arg(rep, report_ptr)))
        return rep

    def sweep_modes_last_encode(self, report_ptr: int = 0):
        """cldn_hip_sweep_modes_last_encode: the points of this codec's most recent encode call (the survivors of a viz call),
        one row per cloud of that call; leaves the state for audit_last_encode and sweep_last_encode as it found it."""
        n = _last_encode_clouds(lib().cldn_hip_sweep_last_encode_clouds, self)
        rep = None if report_ptr else _report((n, self.plan.adaptive_fields), MODE_DTYPE)
        _check(lib().cldn_hip_sweep_modes_last_encode(self._h, *_report_arg(rep, report_ptr)))
        return rep

