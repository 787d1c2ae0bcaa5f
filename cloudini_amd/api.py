"""Python face of the C++ host API (include/cloudini_lib/cloudini.hpp) through include/cloudini_amd_c.h.

Names follow the reference: PointcloudEncoder / PointcloudDecoder / EncodeHeader / DecodeHeader /
MaxCompressedSize and the ROS message converters (cloudini_lib/include/cloudini_lib/cloudini.hpp:126-244,
ros_msg_utils.hpp:175-221). Errors surface as RuntimeError carrying the C++ exception text.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import numpy as np

from .schema import EncodingInfo, EncodingOptions, CompressionOption, FieldType, PointField

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SO = os.path.join(HERE, "lib", "libcloudini_amd.so")


class _Field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("type", C.c_uint8), ("has_resolution", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("resolution", C.c_float)]


class _Info(C.Structure):
    _fields_ = [("fields", C.POINTER(_Field)), ("n_fields", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("point_step", C.c_uint32), ("encoding_opt", C.c_uint8),
                ("compression_opt", C.c_uint8), ("version", C.c_uint8), ("use_threads", C.c_uint8)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    from . import native
    native.lib()  # loads torch's HIP runtime first (if torch is around) and libcloudini_hip.so
    if not os.path.exists(HOST_SO):
        raise ImportError(f"{HOST_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(HOST_SO)
    u8p = C.POINTER(C.c_uint8)
    L.cldn_amd_last_error.restype = C.c_char_p
    L.cldn_LastError.restype = C.c_char_p
    L.cldn_amd_max_compressed_size.restype = C.c_int64
    L.cldn_amd_max_compressed_size.argtypes = [C.POINTER(_Info), C.c_uint64, C.c_int]
    L.cldn_amd_encode_header.restype = C.c_int64
    L.cldn_amd_encode_header.argtypes = [C.POINTER(_Info), C.c_int, u8p, C.c_uint64]
    L.cldn_amd_encode.restype = C.c_int64
    L.cldn_amd_encode.argtypes = [C.POINTER(_Info), u8p, C.c_uint64, u8p, C.c_uint64, C.c_int]
    L.cldn_amd_decode.restype = C.c_int64
    L.cldn_amd_decode.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64, C.c_char_p, C.c_uint64, u8p]
    L.cldn_amd_decode_noheader.restype = C.c_int64
    L.cldn_amd_decode_noheader.argtypes = [C.POINTER(_Info), u8p, C.c_uint64, u8p, C.c_uint64]
    L.cldn_amd_decode_noheader_zeroed.restype = C.c_int64
    L.cldn_amd_decode_noheader_zeroed.argtypes = [C.POINTER(_Info), u8p, C.c_uint64, u8p, C.c_uint64]
    L.cldn_amd_ros_compress.restype = C.c_int64
    L.cldn_amd_ros_compress.argtypes = [u8p, C.c_uint64, C.c_float, C.c_uint8, u8p, C.c_uint64]
    L.cldn_amd_ros_decompress.restype = C.c_int64
    L.cldn_amd_ros_decompress.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64]
    L.cldn_amd_viz_preprocess.restype = C.c_int64
    L.cldn_amd_viz_preprocess.argtypes = [C.POINTER(_Info), u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_float),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.cldn_amd_transcode_directory_on.restype = C.c_int64
    L.cldn_amd_transcode_directory_on.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32,
                                                  C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_double)]
    L.cldn_amd_decode_directory_on.restype = C.c_int64
    L.cldn_amd_decode_directory_on.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int32), C.c_uint32,
                                               C.POINTER(C.c_double)]
    L.cldn_amd_transcode_directory_audit.restype = C.c_int64
    L.cldn_amd_transcode_directory_audit.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32,
                                                     C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                                     C.c_uint32, C.POINTER(C.c_double), C.c_char_p, C.c_uint64]
    L.cldn_amd_transcode_directory_estimate.restype = C.c_int64
    L.cldn_amd_transcode_directory_estimate.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32,
                                                        C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_char_p),
                                                        C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32,
                                                        C.POINTER(C.c_double), C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.cldn_amd_transcode_directory_sweep.restype = C.c_int64
    L.cldn_amd_transcode_directory_sweep.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32,
                                                     C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                                     C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_double), C.c_char_p, C.c_uint64]
    L.cldn_amd_transcode_directory_modes.restype = C.c_int64
    L.cldn_amd_transcode_directory_modes.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32,
                                                     C.POINTER(C.c_int32), C.c_uint32, C.c_int, C.POINTER(C.c_double), C.c_char_p,
                                                     C.c_uint64]
    L.cldn_amd_transcode_directory.restype = C.c_int64
    L.cldn_amd_transcode_directory.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint8, C.c_int, C.c_uint32, C.POINTER(C.c_double)]
    L.cldn_amd_decode_directory_stage2.restype = C.c_int64
    L.cldn_amd_decode_directory_stage2.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_int,
                                                   C.POINTER(C.c_double), C.c_char_p, C.c_uint64]
    L.cldn_amd_decode_directory.restype = C.c_int64
    L.cldn_amd_decode_directory.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_double)]
    L.cldn_amd_stage2_threads.restype = C.c_uint32
    L.cldn_amd_set_stage2_threads.restype = C.c_uint32
    L.cldn_amd_set_stage2_threads.argtypes = [C.c_uint32]
    L.cldn_amd_device_lz4_decode.restype = C.c_int
    L.cldn_amd_set_device_lz4_decode.restype = C.c_int
    L.cldn_amd_set_device_lz4_decode.argtypes = [C.c_int]
    L.cldn_amd_device_zstd_decode.restype = C.c_int
    L.cldn_amd_set_device_zstd_decode.restype = C.c_int
    L.cldn_amd_set_device_zstd_decode.argtypes = [C.c_int]
    L.cldn_amd_device_zstd_decode_count.restype = C.c_uint64
    L.cldn_amd_device_zstd_sequences.restype = C.c_int
    L.cldn_amd_set_device_zstd_sequences.restype = C.c_int
    L.cldn_amd_set_device_zstd_sequences.argtypes = [C.c_int]
    L.cldn_amd_device_zstd_matches.restype = C.c_int
    L.cldn_amd_set_device_zstd_matches.restype = C.c_int
    L.cldn_amd_set_device_zstd_matches.argtypes = [C.c_int]
    L.cldn_amd_device_zstd.restype = C.c_int
    L.cldn_amd_set_device_zstd.restype = C.c_int
    L.cldn_amd_set_device_zstd.argtypes = [C.c_int]
    for name in ("cldn_GetHeaderAsYAML", "cldn_GetHeaderAsYAMLFromDDS", "cldn_ConvertCompressedMsgToPointCloud2Msg",
                 "cldn_DecodeCompressedData", "cldn_DecodeCompressedMessage"):
        getattr(L, name).restype = C.c_uint32
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.cldn_ComputeCompressedSize.restype = C.c_uint32
    L.cldn_ComputeCompressedSize.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
    L.cldn_GetDecompressedSize.restype = C.c_uint32
    L.cldn_GetDecompressedSize.argtypes = [C.c_void_p, C.c_uint32]
    L.cldn_EncodePointcloudMessage.restype = C.c_uint32
    L.cldn_EncodePointcloudMessage.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
    L.cldn_EncodePointcloudData.restype = C.c_uint32
    L.cldn_EncodePointcloudData.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p]
    _lib = L
    return L


def _c_info(info) -> Tuple[_Info, object]:
    arr = (_Field * max(1, len(info.fields)))()
    keep = []
    for i, f in enumerate(info.fields):
        nm = f.name.encode()
        keep.append(nm)
        arr[i].name = nm
        arr[i].offset = int(f.offset)
        arr[i].type = int(f.type)
        arr[i].has_resolution = 0 if f.resolution is None else 1
        arr[i].resolution = 0.0 if f.resolution is None else float(f.resolution)
    ci = _Info(arr, len(info.fields), int(info.width), int(info.height), int(info.point_step), int(info.encoding_opt),
               int(info.compression_opt), int(info.version), 1 if info.use_threads else 0)
    return ci, (arr, keep)


def _u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _check(r: int) -> int:
    if r < 0:
        raise RuntimeError(lib().cldn_amd_last_error().decode(errors="replace"))
    return r


def stage2_threads() -> int:
    """Threads one encode()/decode() call may use for LZ4/ZSTD, the caller included (bounded pool)."""
    return int(lib().cldn_amd_stage2_threads())


def set_stage2_threads(n: int) -> int:
    return int(lib().cldn_amd_set_stage2_threads(int(n)))


def device_lz4() -> bool:
    return bool(lib().cldn_amd_device_lz4())


def set_device_lz4(on) -> int:
    """LZ4 streams with stage 2 on the GPU (valid LZ4 blocks, not lz4's own bytes): False / 0 off, True / 1 on, 2 = the FAST
    parameters (4 KiB windows). Returns the level in effect."""
    return int(lib().cldn_amd_set_device_lz4(int(on)))


def device_lz4_decode() -> bool:
    return bool(lib().cldn_amd_device_lz4_decode())


def set_device_lz4_decode(on) -> bool:
    """PointcloudDecoder.decode of LZ4 messages (wire version >= 3) with stage 2 undone on the GPU (cldn_hip_decode_lz4) instead
    of liblz4 on the host pool. Off by default. Returns the value in effect."""
    return bool(lib().cldn_amd_set_device_lz4_decode(1 if on else 0))


def device_zstd_decode() -> bool:
    return bool(lib().cldn_amd_device_zstd_decode())


def set_device_zstd_decode(on) -> bool:
    """PointcloudDecoder.decode of ZSTD messages (wire version >= 3) whose frames carry no sequences -- what set_device_zstd
    writes -- with stage 2 undone on the GPU (cldn_hip_decode_zstd); every other message takes the host route as before.
    Measured: a single message is 6 to 20 times slower this way than on 16 host threads; the device decoder pays for
    device-resident batches (native.Codec.decode_zstd_device), not for single host messages. Off by default. Returns the value in
    effect."""
    return bool(lib().cldn_amd_set_device_zstd_decode(1 if on else 0))


def device_zstd_sequences() -> bool:
    return bool(lib().cldn_amd_device_zstd_sequences())


def set_device_zstd_sequences(on) -> bool:
    """With set_device_zstd_decode on: ZSTD messages whose frames carry sequences -- what libzstd writes at every level -- take
    the device route too (cldn_hip_codec_set_zstd_sequences); fall-backs stay silent.
    Measured: a single message is 11 to 23 times slower this way than libzstd on 16 host threads (1 M XYZI points:
    16.4 ms against 1.5 ms), so leave it off for host messages. Off by default.
    Returns the value in effect."""
    return bool(lib().cldn_amd_set_device_zstd_sequences(1 if on else 0))


def device_zstd_decode_count() -> int:
    """Messages that took the device route through set_device_zstd_decode since the library was loaded (fall-backs are silent)."""
    return int(lib().cldn_amd_device_zstd_decode_count())


def device_zstd_matches() -> bool:
    return bool(lib().cldn_amd_device_zstd_matches())


def set_device_zstd_matches(on) -> bool:
    """On top of set_device_zstd(True): the device's ZSTD frames carry sequences from its match search
    (cldn_hip_codec_set_zstd_matches). Pays where the stage-1 bytes repeat (ring fields, lossless float64 stamps); token streams
    stay as they are. Off by default; returns the value in effect."""
    return bool(lib().cldn_amd_set_device_zstd_matches(1 if on else 0))


def device_zstd() -> bool:
    return bool(lib().cldn_amd_device_zstd())


def set_device_zstd(on) -> bool:
    """ZSTD streams with stage 2 on the GPU: PointcloudEncoder.encode writes frames of literal-only blocks (valid ZSTD frames
    that any decoder reads, not libzstd's bytes; larger where ZSTD finds matches). Off by default. Returns the value in effect."""
    return bool(lib().cldn_amd_set_device_zstd(1 if on else 0))


def _device_list(devices):
    if not devices:
        return None, 0
    arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    return arr, len(devices)


def transcode_directory(in_dir: str, out_dir: str, resolution: float = 0.001, compression_opt: int = 2,
                        viz_lossy: bool = False, batch_messages: int = 64, devices=None, audit: bool = False,
                        audit_limits=None, sweep=None, modes=None, estimate: bool = False) -> dict:
    """Batch transcoder (include/cloudini_amd/batch_transcoder.hpp): every CDR PointCloud2 file of in_dir ->
    CompressedPointCloud2 file of the same name in out_dir. `devices`: GPUs to spread the batches over (one GPU stage per
    entry; None = the current device). Returns the statistics. audit=True: every encode call is audited on the device
    (cldn_hip_audit_last_encode) and the per-field summary comes back under "audit" -- a list of dicts (name, is_float,
    n_bitwise_diff, n_class_diff, n_over_limit, max_abs_err, first_bad_message); audit_limits: {field name: limit} for the
    fields that should not be held to their resolution. sweep={field name: [resolutions]} ("xyz" names x, y and z; at most 16
    per name): the points of every encode call are swept on the device (cldn_hip_sweep_last_encode) and "sweep" holds, per
    field name and resolution, a dict (name, resolution, bytes, points, n_class_diff, n_over_limit, max_abs_err) -- what the
    field would cost in stage-1 bytes and lose at that resolution. The files are those of a run without it.
    estimate=True (needs sweep): "estimate" holds {"own_bytes", "stage1_bytes", "actual_bytes", "fields": [name, resolution,
    bytes]} -- per field name and resolution the order-0 entropy of the messages' streams if that field alone had that
    resolution (cldn_hip_sweep_hist_last_encode, cldn_hip_stream_hist_last_encode): what ZSTD level 1 makes of them.
    modes="report": the adaptive integer modes of every encode call's points are swept on the device
    (cldn_hip_sweep_modes_last_encode) and "modes" holds {"reencoded_runs", "fields": [per integer field name: clouds, bytes
    under DeltaVarint / Palette / Rle / DeltaRle, clouds probed into and best in each mode, saved_bytes]}; the files are those
    of a run without it. modes="best": a schema run in which a cloud's best mode differs from the probed one is encoded again
    with the best modes forced -- those messages are NOT the reference encoder's bytes, but valid streams that every Cloudini
    decoder decodes to the same points. One of audit, sweep and modes per call."""
    if estimate and not sweep:
        raise ValueError("transcode_directory: estimate needs sweep")
    st = (C.c_double * 8)()
    dv, nd = _device_list(devices)
    keys = ("messages", "points", "input_bytes", "output_bytes", "gpu_batches", "seconds_total", "seconds_gpu", "seconds_stage2")
    if modes not in (None, "off", "report", "best"):
        raise ValueError("transcode_directory: modes is 'off', 'report' or 'best'")
    if modes in ("report", "best"):
        if audit or sweep:
            raise ValueError("transcode_directory: audit, sweep and modes are separate calls")
        import json
        text = C.create_string_buffer(1 << 20)
        _check(lib().cldn_amd_transcode_directory_modes(in_dir.encode(), out_dir.encode(), resolution, compression_opt,
                                                        1 if viz_lossy else 0, batch_messages, dv, nd, 1 if modes == "best" else 0,
                                                        st, text, len(text)))
        out = dict(zip(keys, [float(x) for x in st]))
        out["modes"] = json.loads(text.value.decode())
        return out
    if sweep:
        if audit:
            raise ValueError("transcode_directory: audit and sweep are separate calls")
        import json
        names = (C.c_char_p * len(sweep))(*[k.encode() for k in sweep])
        sizes = (C.c_uint32 * len(sweep))(*[len(v) for v in sweep.values()])
        flat = [float(r) for v in sweep.values() for r in v]
        values = (C.c_float * max(1, len(flat)))(*flat)
        text = C.create_string_buffer(1 << 20)
        if estimate:
            text2 = C.create_string_buffer(1 << 20)
            _check(lib().cldn_amd_transcode_directory_estimate(in_dir.encode(), out_dir.encode(), resolution, compression_opt,
                                                               1 if viz_lossy else 0, batch_messages, dv, nd, names, sizes, values,
                                                               len(sweep), st, text, len(text), text2, len(text2)))
        else:
            _check(lib().cldn_amd_transcode_directory_sweep(in_dir.encode(), out_dir.encode(), resolution, compression_opt,
                                                            1 if viz_lossy else 0, batch_messages, dv, nd, names, sizes, values,
                                                            len(sweep), st, text, len(text)))
        out = dict(zip(keys, [float(x) for x in st]))
        out["sweep"] = json.loads(text.value.decode())
        if estimate:
            out["estimate"] = json.loads(text2.value.decode())
        return out
    if not audit:
        _check(lib().cldn_amd_transcode_directory_on(in_dir.encode(), out_dir.encode(), resolution, compression_opt,
                                                     1 if viz_lossy else 0, batch_messages, dv, nd, st))
        return dict(zip(keys, [float(x) for x in st]))
    import json
    limits = dict(audit_limits or {})
    names = (C.c_char_p * max(1, len(limits)))(*[k.encode() for k in limits])
    values = (C.c_double * max(1, len(limits)))(*[float(v) for v in limits.values()])
    text = C.create_string_buffer(1 << 20)
    _check(lib().cldn_amd_transcode_directory_audit(in_dir.encode(), out_dir.encode(), resolution, compression_opt,
                                                    1 if viz_lossy else 0, batch_messages, dv, nd, names, values, len(limits), st,
                                                    text, len(text)))
    out = dict(zip(keys, [float(x) for x in st]))
    out["audit"] = json.loads(text.value.decode())
    return out


def decode_directory(in_dir: str, out_dir: str, batch_messages: int = 64, devices=None, device_stage2: bool = False) -> dict:
    """The way back: every CDR CompressedPointCloud2 file of in_dir -> PointCloud2 file of the same name in out_dir
    (batched GPU decode). Returns the statistics. device_stage2 (TranscodeOptions::device_stage2_decode): LZ4 and ZSTD stage 2
    is undone on the device too -- the same files; device_stage2_chunks, host_stage2_chunks and device_stage2_retries tell
    what happened (all 0 without the option)."""
    import json
    st = (C.c_double * 8)()
    dv, nd = _device_list(devices)
    text = C.create_string_buffer(1 << 10)
    _check(lib().cldn_amd_decode_directory_stage2(in_dir.encode(), out_dir.encode(), batch_messages, dv, nd, 1 if device_stage2 else 0,
                                                  st, text, len(text)))
    keys = ("messages", "points", "input_bytes", "output_bytes", "gpu_batches", "seconds_total", "seconds_gpu", "seconds_stage2")
    out = dict(zip(keys, [float(x) for x in st]))
    out.update(json.loads(text.value.decode()))
    return out


def MaxCompressedSize(info, points_count: int, include_header: bool = True) -> int:
    ci, _keep = _c_info(info)
    return _check(lib().cldn_amd_max_compressed_size(C.byref(ci), points_count, 1 if include_header else 0))


def EncodeHeader(info, binary: bool = False) -> bytes:
    ci, _keep = _c_info(info)
    out = np.empty(1 << 16, dtype=np.uint8)
    n = _check(lib().cldn_amd_encode_header(C.byref(ci), 1 if binary else 0, _ptr(out), out.size))
    return out[:n].tobytes()


def parse_yaml_info(yaml: str, version: int) -> EncodingInfo:
    """EncodingInfoToYAML text -> EncodingInfo (Python side, for the tests)."""
    info = EncodingInfo(fields=[], version=version)
    cur = None
    for line in yaml.splitlines():
        s = line.strip()
        if not s or s == "fields:":
            continue
        if s.startswith("- "):
            cur = PointField("")
            info.fields.append(cur)
            s = s[2:]
        k, _, v = s.partition(":")
        k, v = k.strip(), v.strip()
        if cur is None:
            if k in ("width", "height", "point_step"):
                setattr(info, k, int(v))
            elif k == "encoding_opt":
                info.encoding_opt = EncodingOptions[v]
            elif k == "compression_opt":
                info.compression_opt = CompressionOption[v]
            elif k == "encoding_config":
                info.encoding_config = v
        else:
            if k == "name":
                cur.name = v
            elif k == "offset":
                cur.offset = int(v)
            elif k == "type":
                cur.type = FieldType[v]
            elif k == "resolution":
                cur.resolution = None if v == "null" else float(np.float32(v))
    return info


class PointcloudEncoder:
    def __init__(self, info: EncodingInfo):
        self.info = info

    def getHeader(self) -> bytes:
        return EncodeHeader(self.info)

    def encode(self, cloud, write_header: bool = True) -> np.ndarray:
        data = _u8(cloud)
        step = int(self.info.point_step)
        points = data.size // step if step else 0
        ci, _keep = _c_info(self.info)
        cap = MaxCompressedSize(self.info, points, True)
        out = np.empty(cap, dtype=np.uint8)
        n = _check(lib().cldn_amd_encode(C.byref(ci), _ptr(data) if data.size else None, data.size, _ptr(out), cap,
                                         1 if write_header else 0))
        return out[:n].copy()


class PointcloudDecoder:
    def decode_stream(self, stream, fill: int = 0):
        """Full stream (header + chunks) -> (decoded bytes, EncodingInfo of the header)."""
        st = _u8(stream)
        yaml = C.create_string_buffer(1 << 16)
        ver = C.c_uint8(0)
        # first pass with a zero-size buffer is not possible (decode needs the output); size it from the header text
        hdr_end = st.tobytes().find(b"\0")
        info = None
        if st[:10].tobytes() == b"CLOUDINI_V" and hdr_end > 0 and st[12] == 0x0A:
            info = parse_yaml_info(st[13:hdr_end].tobytes().decode(), int(st[10:12].tobytes()))
            size = info.width * info.height * info.point_step
        else:
            size = 1 << 26
        out = np.full(max(1, size), fill, dtype=np.uint8)
        n = _check(lib().cldn_amd_decode(_ptr(st), st.size, _ptr(out), out.size, yaml, len(yaml), C.byref(ver)))
        return out[:n], parse_yaml_info(yaml.value.decode(), ver.value)

    def decode(self, info: EncodingInfo, data, fill: int = 0, output_is_zero: bool = False) -> np.ndarray:
        """PointcloudDecoder::decode(info, compressed_data (no header), output). output_is_zero: the buffer is handed over
        all zeros (decodeInto(..., true): what decode(info, data, std::vector&) does for a vector that arrives empty)."""
        st = _u8(data)
        size = int(info.width) * int(info.height) * int(info.point_step)
        out = np.full(max(1, size), 0 if output_is_zero else fill, dtype=np.uint8)
        ci, _keep = _c_info(info)
        call = lib().cldn_amd_decode_noheader_zeroed if output_is_zero else lib().cldn_amd_decode_noheader
        n = _check(call(C.byref(ci), _ptr(st) if st.size else None, st.size, _ptr(out), size))
        return out[:n]


def ros_compress(dds, resolution: float, compression_opt: int) -> np.ndarray:
    msg = _u8(dds)
    out = np.empty(msg.size * 3 + (1 << 20), dtype=np.uint8)
    n = _check(lib().cldn_amd_ros_compress(_ptr(msg), msg.size, resolution, compression_opt, _ptr(out), out.size))
    return out[:n].copy()


def ros_decompress(dds, capacity: int) -> np.ndarray:
    msg = _u8(dds)
    out = np.empty(capacity, dtype=np.uint8)
    n = _check(lib().cldn_amd_ros_decompress(_ptr(msg), msg.size, _ptr(out), out.size))
    return out[:n].copy()


def applyVizLossyPreprocessing(info, cloud):
    """cloudini_ros::applyVizLossyPreprocessing on a bare point buffer -> (surviving bytes, per-field resolution
    afterwards (None = none), width, height)."""
    data = _u8(cloud)
    ci, _keep = _c_info(info)
    out = np.empty(max(1, data.size), dtype=np.uint8)
    res = (C.c_float * max(1, len(info.fields)))()
    w, h = C.c_uint32(0), C.c_uint32(0)
    n = _check(lib().cldn_amd_viz_preprocess(C.byref(ci), _ptr(data) if data.size else None, data.size, _ptr(out),
                                             out.size, res, C.byref(w), C.byref(h)))
    return out[:n].copy(), [None if x != x else float(x) for x in list(res)[: len(info.fields)]], int(w.value), int(h.value)


# ---- adaptive integer modes on raw clouds (cldn_hip_sweep_modes_*, cldn_hip_codec_force_modes_per_cloud) -----------------

def sweep_modes(info, clouds):
    """Per cloud and adaptive integer field of `info`'s schema: the section bytes under each of the four V5 modes, the mode the
    reference's probe commits and the best mode over the whole cloud (native.MODE_DTYPE, shape (n_clouds, adaptive fields))."""
    from . import native
    return native.Codec(native.Plan(info)).sweep_modes_host(clouds)


def encode_stage1_with_modes(info, clouds, modes):
    """Framed stage-1 streams of `clouds` with the adaptive integer modes forced per cloud (modes: (n_clouds, adaptive fields),
    e.g. sweep_modes(...)["best_mode"]). Valid Cloudini streams, not the reference encoder's bytes where a mode differs."""
    from . import native
    codec = native.Codec(native.Plan(info))
    codec.force_modes_per_cloud(modes)
    return codec.encode_host(clouds)[0]


# ---- byte histograms for the stage-2 estimate (cldn_hip_sweep_hist_*, cldn_hip_stream_hist, cldn_hip_hist_entropy_bytes) --

def sweep_hist(info, clouds, resolutions):
    """Per cloud, field and candidate resolution (resolutions: (n_fields, n_candidates), 0 = skip): the 256-bin histogram of the
    bytes of the field's tokens at that resolution; uint64, shape (n_clouds, n_fields, n_candidates, 256). Zero for fields
    without a lossy float encoder."""
    from . import native
    return native.Codec(native.Plan(info)).sweep_hist_clouds_host(clouds, resolutions)


def stream_hist(info, streams):
    """The 256-bin histogram of the bytes of each stream (uint64, shape (n_streams, 256)), counted on the device."""
    from . import native
    return native.Codec(native.Plan(info)).stream_hist_host(streams)


def hist_entropy_bytes(hist) -> float:
    """Order-0 entropy, in bytes, of the bytes a 256-bin histogram counts: what ZSTD level 1 makes of them while literals
    dominate. With stream_hist - sweep_hist[f][own] + sweep_hist[f][candidate]: the estimate for field f at the candidate."""
    from . import native
    return native.hist_entropy_bytes(hist)
