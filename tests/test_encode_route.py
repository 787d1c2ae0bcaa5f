"""cloudini_amd/csrc/stage1_encode_route.h -- which kernels encode a batch, and the geometry of its slots -- compiled with g++ and
checked against a table of expected kernel sequences and scalar fields, on the CPU. The table was filled by reading the
launcher and the ABI arithmetic the route replaced; tools/encode_route_trace.py checks it against kernel traces of both
(profiles/r14_a_encode_route_kernels.txt)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QF32, LF32, LF64, INT, COPY, XOR32, XOR64, GOR = range(8)  # DevOp::kind (stage1_device.h)
REGULAR = ("none", "wide", "pieces", "fixed", "fixed_direct", "generic")
PREPASS = ("none", "gorilla_windows", "gorilla_tokens", "wide_groups")
PROBE = ("none", "pieces", "fast", "wide")
CLOSE = ("none", "finish", "chunk_sizes", "offsets_memset")
FIELDS = ("regular", "generic_kernel", "variant", "lanes", "loadw", "unal", "l3", "tail", "tail_op", "prepass", "prepass_groups", "probe",
          "n_probe", "pieces_lds", "writes_caller_modes", "fixed_bytes", "fixed_total", "sections", "fused_field", "append", "sec_grid",
          "close", "finish_threads", "finish_bpv", "finish_lds", "splits", "intra", "kernel_clears", "piece_pts", "piece_wgs", "piece_stride",
          "wave_stride", "subs", "sub_points", "sub_stride", "segs_per_chunk", "reg_stride", "slot_stride")
LISTS = ("runs", "pal16", "pal32", "pal64")
# k_encode_fused<lanes, loadw, unal, l3, tail>: the instantiations that are built
FUSED_VARIANTS = [(3, 3, 0, 3, 0), (3, 4, 0, 3, 0), (3, 8, 0, 3, 0), (4, 4, 0, 3, 0), (4, 8, 0, 3, 0), (4, 8, 0, 4, 0), (3, 4, 1, 3, 0),
                  (3, 8, 1, 3, 0), (4, 5, 1, 3, 0), (4, 8, 1, 3, 0), (3, 4, 0, 3, 1), (3, 8, 0, 3, 1), (4, 8, 0, 3, 1), (4, 8, 0, 4, 1),
                  (3, 4, 1, 3, 1), (3, 8, 1, 3, 1), (4, 8, 1, 3, 1)]
FINISH_VARIANTS = {(256, 0): 0, (512, 2): 24848, (512, 4): 41232, (1024, 2): 24848, (1024, 4): 41232}  # (threads, bpv): LDS
SECTION_STRIDE = 409600

FUSED, GENERIC, FIXED, FIN, SECS = ["k_encode_fused"], ["k_encode_regular"], ["k_encode_fixed"], ["k_finish"], ["k_encode_sections"]
RUNS, PAL32, PAL64, PROBE_FAST = ["k_section_fast"], ["k_section_palette32"], ["k_section_palette"], ["k_probe_fast"]
LDS_SMALL, LDS_TAIL3, LDS_TAIL4, LDS_PROBE32 = 18320, 50576, 45520, 24848  # piece kernel: 4 regions (+ 16); the 32-bit probe's table


def xyz(first=0):
    return [(QF32, 4, first), (QF32, 4, first + 4), (QF32, 4, first + 8)]


def xyzw(first=0, w=12):
    return xyz(first) + [(QF32, 4, first + w)]


# fields: (FieldType, offset, has resolution)
XYZ_F = [(7, 0, 1), (7, 4, 1), (7, 8, 1)]
XYZW_F = XYZ_F + [(7, 12, 1)]
XYZI = dict(step=16, ops=xyz(), adaptive=[(2, 12)])
XYZI_F = XYZ_F + [(4, 12, 0)]
XYZ = dict(step=12, ops=xyz())
TWO_FLOATS = [(LF32, 4, 0), (LF32, 4, 4)]
TWO_FLOATS_F = [(7, 0, 1), (7, 4, 1)]
HEADLINE = dict(regular="pieces", variant=1, probe="pieces", n_probe=1, pieces_lds=LDS_SMALL, writes_caller_modes=1, fused_field=0,
                finish_threads=1024, finish_bpv=2, splits=4, kernel_clears=1, intra=0, piece_pts=504, piece_wgs=17, piece_stride=7680,
                wave_stride=7680, subs=17, sub_points=504, sub_stride=30720, segs_per_chunk=19, reg_stride=522240, slot_stride=931840,
                runs=[0], pal16=[], pal32=[], pal64=[], append=0, sec_grid=2, close="finish")


def row(name, kernels, step, ops, adaptive=(), fields=None, expect=None, **call):
    return dict(name=name, kernels=kernels, step=step, ops=list(ops), adaptive=list(adaptive), fields=fields, expect=expect or {}, call=call)


def variant(*v):
    return FUSED_VARIANTS.index(v)


# call: n_chunks (2), n_clouds (1), pipeline, wide, table, lz4, residue (of the points' address), forced (the forced modes' hint
# bits per field), hints (per field; 0xF), new_zero_block, out_capacity, wide_adaptive, wide_gorilla, max_regular_bytes.
# fields / lossless / data: what tools/encode_route_trace.py builds the row's plan and points from (data: "walk" / "few" for
# all integer fields, or one of them per field). Every row the C ABI can produce at up to 1024 chunks has `fields` and is traced
# on the GPU; gpu=0 rows say in `why` what keeps them on the CPU.
ROWS = [
    # ---- the 17 instantiations of the piece kernel, by a layout that selects each ----
    row("xyzi", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, expect=HEADLINE),
    row("xyz", FUSED + FIN, **XYZ, fields=XYZ_F,
        expect=dict(regular="pieces", variant=variant(3, 3, 0, 3, 0), probe="none", n_probe=0, pieces_lds=LDS_SMALL, fused_field=-1,
                    finish_threads=256, finish_bpv=0, splits=16, kernel_clears=1, segs_per_chunk=17, slot_stride=522240, sections=0)),
    row("xyz_in_16_bytes", FUSED + FIN, 16, xyz(), fields=XYZ_F,
        expect=dict(variant=variant(3, 3, 0, 3, 0), pieces_lds=LDS_SMALL, segs_per_chunk=17, slot_stride=522240, probe="none", kernel_clears=1)),
    row("xyz_u16_at_20", FUSED + RUNS + SECS + FIN, 32, xyz(), [(2, 20)], fields=XYZ_F + [(4, 20, 0)],
        expect=dict(variant=variant(3, 8, 0, 3, 0), pieces_lds=LDS_SMALL, probe="pieces", n_probe=1, fused_field=0, runs=[0], pal16=[],
                    segs_per_chunk=19, slot_stride=931840)),
    row("xyzw", FUSED + FIN, 16, xyzw(), fields=XYZW_F,
        expect=dict(variant=variant(4, 4, 0, 3, 0), piece_pts=378, piece_wgs=22, subs=22, piece_stride=7680, sub_stride=30720,
                    pieces_lds=LDS_SMALL, reg_stride=22 * 30720)),
    row("xyzw_u16", FUSED + RUNS + SECS + FIN, 32, xyzw(), [(2, 16)], fields=XYZW_F + [(4, 16, 0)],
        expect=dict(variant=variant(4, 8, 0, 3, 0), pieces_lds=LDS_SMALL, fused_field=0, runs=[0], pal16=[], subs=22, segs_per_chunk=24,
                    reg_stride=675840, slot_stride=1085440)),
    row("pcl_xyz_pad_i", FUSED + FIN, 32, xyzw(w=16), fields=XYZ_F + [(7, 16, 1)],
        expect=dict(variant=variant(4, 8, 0, 4, 0), piece_wgs=22, pieces_lds=LDS_SMALL, slot_stride=675840, segs_per_chunk=22)),
    row("xyz_residue_1", FUSED + FIN, **XYZ, fields=XYZ_F, residue=1,
        expect=dict(variant=variant(3, 4, 1, 3, 0), pieces_lds=LDS_SMALL, piece_stride=7680, slot_stride=522240, kernel_clears=1)),
    row("xyz_residue_2", FUSED + FIN, **XYZ, fields=XYZ_F, residue=2,
        expect=dict(variant=variant(3, 4, 1, 3, 0), pieces_lds=LDS_SMALL, piece_stride=7680, slot_stride=522240, kernel_clears=1)),
    row("xyz_residue_3", FUSED + FIN, **XYZ, fields=XYZ_F, residue=3,
        expect=dict(variant=variant(3, 4, 1, 3, 0), pieces_lds=LDS_SMALL, piece_stride=7680, slot_stride=522240, kernel_clears=1)),
    row("packed_18_u16_u32", FUSED + RUNS + PAL32 + SECS + FIN, 18, xyz(), [(2, 12), (4, 14)], fields=XYZI_F + [(6, 14, 0)],
        expect=dict(variant=variant(3, 8, 1, 3, 0), probe="pieces", n_probe=2, pieces_lds=LDS_PROBE32, fused_field=0, runs=[0, 1], pal32=[1],
                    finish_threads=1024, finish_bpv=2, segs_per_chunk=21)),
    row("packed_18_xyzw_u16", FUSED + RUNS + SECS + FIN, 18, xyzw(), [(2, 16)], fields=XYZW_F + [(4, 16, 0)],
        expect=dict(variant=variant(4, 5, 1, 3, 0), pieces_lds=LDS_SMALL, probe="pieces", fused_field=0, runs=[0], pal16=[], slot_stride=1085440)),
    row("packed_22_xyzw_u16_u32", FUSED + RUNS + PAL32 + SECS + FIN, 22, xyzw(), [(2, 16), (4, 18)], fields=XYZW_F + [(4, 16, 0), (6, 18, 0)],
        expect=dict(variant=variant(4, 8, 1, 3, 0), pieces_lds=LDS_PROBE32, n_probe=2, fused_field=0, runs=[0, 1], pal16=[], pal32=[1],
                    segs_per_chunk=26, slot_stride=675840 + 2 * 409600)),
    row("xyz_copy4", FUSED + FIN, 16, xyz() + [(COPY, 4, 12)], fields=XYZ_F + [(7, 12, 0)],
        expect=dict(variant=variant(3, 4, 0, 3, 1), tail_op=3, pieces_lds=LDS_TAIL3, piece_stride=12800, sub_stride=51200, kernel_clears=1)),
    row("xyz_f64_step_32", FUSED + FIN, 32, xyz() + [(LF64, 8, 16)], fields=XYZ_F + [(8, 16, 1)], expect=dict(variant=variant(3, 8, 0, 3, 1), tail_op=3)),
    row("xyzw_f32_step_32", FUSED + FIN, 32, xyzw() + [(LF32, 4, 16)], gpu=0, why="five leading FLOAT32 fields with a resolution form no FloatN group: no plan of the ABI has 4 lanes + a lossy float32",
        expect=dict(variant=variant(4, 8, 0, 3, 1), tail_op=4, pieces_lds=LDS_TAIL4, piece_stride=11520)),
    row("xyzw_copy4_step_32", FUSED + FIN, 32, xyzw() + [(COPY, 4, 16)], fields=XYZW_F + [(7, 16, 0)], expect=dict(variant=variant(4, 8, 0, 3, 1))),
    row("pcl_gorilla", ["k_gorilla_windows"] + FUSED + FIN, 32, xyzw(w=16) + [(GOR, 8, 24)], fields=XYZ_F + [(7, 16, 1), (8, 24, 0)],
        expect=dict(variant=variant(4, 8, 0, 4, 1), tail_op=4, prepass="gorilla_windows", kernel_clears=0)),
    row("xyz_copy2_step_14", FUSED + FIN, 14, xyz() + [(COPY, 2, 12)], gpu=0,
        why="a 2-byte field behind lossy floats is an adaptive integer field, not a raw copy", expect=dict(variant=variant(3, 4, 1, 3, 1))),
    # TAIL layouts whose loaded dwords reach past the point: the guarded UNAL instantiation, though everything is aligned
    row("xyz_f64_step_24", FUSED + FIN, 24, xyz() + [(LF64, 8, 16)], fields=XYZ_F + [(8, 16, 1)], expect=dict(variant=variant(3, 8, 1, 3, 1))),
    row("xyz_u16_f32_step_20", FUSED + RUNS + SECS + FIN, 20, xyz() + [(LF32, 4, 16)], [(2, 12)], fields=XYZI_F + [(7, 16, 1)],
        expect=dict(variant=variant(3, 8, 1, 3, 1), tail_op=3, probe="pieces", fused_field=0)),
    row("xyzw_f32_step_20", FUSED + FIN, 20, xyzw() + [(LF32, 4, 16)], gpu=0, why="five leading FLOAT32 fields with a resolution form no FloatN group: no plan of the ABI has 4 lanes + a lossy float32", expect=dict(variant=variant(4, 8, 1, 3, 1))),
    row("xyzw_copy4_step_20", FUSED + FIN, 20, xyzw() + [(COPY, 4, 16)], fields=XYZW_F + [(7, 16, 0)], expect=dict(variant=variant(4, 8, 1, 3, 1))),
    # ---- layouts that fall to the generic kernel (and two that look as if they did) ----
    row("field_in_front_with_tail", GENERIC + PROBE_FAST + RUNS + SECS + FIN, 20, xyz(4) + [(COPY, 4, 16)], [(2, 0)],
        fields=[(7, 4, 1), (7, 8, 1), (7, 12, 1), (7, 16, 0), (4, 0, 0)],
        expect=dict(regular="generic", variant=-1, piece_pts=0, probe="fast", fused_field=0, subs=32, kernel_clears=0, generic_kernel=0)),
    row("field_in_front", FUSED + RUNS + SECS + FIN, 16, xyz(4), [(2, 0)], fields=[(7, 4, 1), (7, 8, 1), (7, 12, 1), (4, 0, 0)],  # loadw == lanes: the kernel reads every field directly
        expect=dict(regular="pieces", variant=variant(3, 3, 0, 3, 0), probe="pieces")),
    row("xyz_u64_odd_offset_unaligned", GENERIC + PROBE_FAST + PAL64 + SECS + FIN, 22, xyz(), [(8, 14)], fields=XYZ_F + [(10, 14, 0)],
        expect=dict(regular="generic", variant=-1, probe="fast", fused_field=-1, runs=[], pal64=[0], finish_threads=256, finish_bpv=0, splits=16)),
    row("xyz_u16_at_40_unaligned", GENERIC + PROBE_FAST + RUNS + SECS + FIN, 42, xyz(), [(2, 40)], fields=XYZ_F + [(4, 40, 0)],
        expect=dict(regular="generic", variant=-1)),
    # (4 unaligned lanes without an integer field would load 4 dwords; the unaligned 4-lane kernels are built for 5 and 8)
    row("xyzw_residue_2", GENERIC + FIN, 16, xyzw(), fields=XYZW_F, residue=2, expect=dict(regular="generic", variant=-1, kernel_clears=0)),
    # ---- fixed-size streams ----
    row("4_xor", FIXED + ["k_fixed_offsets"], 16, [(XOR32, 4, 4 * k) for k in range(4)], fields=[(7, 4 * k, 0) for k in range(4)], lossless=1,
        expect=dict(regular="fixed_direct", fixed_bytes=16, fixed_total=4 * 2 + 16 * 32868, close="none", subs=32, sub_points=1024,
                    sub_stride=16640, kernel_clears=0)),
    row("4_xor_one_byte_short", FIXED + FIN, 16, [(XOR32, 4, 4 * k) for k in range(4)], out_capacity=4 * 2 + 16 * 32868 - 1, gpu=0,
        why="the ABI refuses a capacity below the stage-1 bound, which is larger",
        expect=dict(regular="fixed", fixed_bytes=16, close="finish", finish_threads=256, splits=16)),
    row("4_xor_exact_capacity", FIXED + ["k_fixed_offsets"], 16, [(XOR32, 4, 4 * k) for k in range(4)], out_capacity=4 * 2 + 16 * 32868, gpu=0,
        why="the ABI refuses a capacity below the stage-1 bound, which is larger",
        expect=dict(regular="fixed_direct")),
    row("4_xor_table", FIXED + ["k_chunk_sizes"], 16, [(XOR32, 4, 4 * k) for k in range(4)], fields=[(7, 4 * k, 0) for k in range(4)], lossless=1,
        table=1, expect=dict(regular="fixed", close="chunk_sizes", intra=0)),
    # (adaptive integer fields exist in lossy plans only: there a FLOAT32 field without a resolution is a raw copy)
    row("4_copy_u16", FIXED + PROBE_FAST + RUNS + SECS + FIN, 18, [(COPY, 4, 4 * k) for k in range(4)], [(2, 16)],
        fields=[(7, 4 * k, 0) for k in range(4)] + [(4, 16, 0)],
        expect=dict(regular="fixed", probe="fast", fused_field=0, finish_threads=1024, finish_bpv=2)),
    # ---- the generic kernel's two instantiations ----
    row("2_floats_step_256", GENERIC + FIN, 256, TWO_FLOATS, fields=TWO_FLOATS_F, expect=dict(regular="generic", generic_kernel=0)),
    row("2_floats_step_257", GENERIC + FIN, 257, TWO_FLOATS, fields=TWO_FLOATS_F, expect=dict(regular="generic", generic_kernel=1)),
    row("xyz_gorilla_step_32_generic", ["k_gorilla_tokens"] + GENERIC + FIN, 32, xyz() + [(GOR, 8, 16)], fields=XYZ_F + [(8, 16, 0)], pipeline=1,
        expect=dict(regular="generic", prepass="gorilla_tokens")),
    # ---- where the modes are decided ----
    row("xyz_u32", FUSED + RUNS + SECS + FIN, 16, xyz(), [(4, 12)], fields=XYZ_F + [(6, 12, 0)],
        expect=dict(variant=variant(3, 4, 0, 3, 0), probe="pieces", pieces_lds=LDS_PROBE32, fused_field=0, finish_threads=1024, finish_bpv=4)),
    row("xyz_u64", FUSED + PROBE_FAST + PAL64 + SECS + FIN, 24, xyz(), [(8, 16)], fields=XYZ_F + [(10, 16, 0)],
        expect=dict(variant=variant(3, 3, 0, 3, 0), probe="fast", n_probe=0, pieces_lds=LDS_SMALL, writes_caller_modes=0, fused_field=-1,
                    pal64=[0], runs=[], finish_threads=256, kernel_clears=1)),
    row("xyzi_forced_palette", FUSED + SECS + FIN, **XYZI, fields=XYZI_F, forced=[0x2],
        expect=dict(probe="none", n_probe=0, writes_caller_modes=0, fused_field=0, runs=[], pal16=[], kernel_clears=1)),
    row("xyzi_forced_delta_varint", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, forced=[0x1],
        expect=dict(probe="none", fused_field=-1, runs=[0], finish_threads=256, splits=16)),
    row("xyzi_2p20_minus_1_clouds", FUSED + RUNS + SECS + FIN, **XYZI, n_chunks=(1 << 20) - 1, n_clouds=(1 << 20) - 1, gpu=0, why="2^20 clouds",
        expect=dict(probe="pieces", n_probe=(1 << 20) - 1, finish_threads=512, finish_bpv=2, splits=1, sec_grid=256)),
    row("xyzi_2p20_clouds", FUSED + PROBE_FAST + RUNS + SECS + FIN, **XYZI, n_chunks=1 << 20, n_clouds=1 << 20, gpu=0, why="2^20 clouds",
        expect=dict(probe="fast", n_probe=0, writes_caller_modes=0)),
    # ---- the field k_finish builds, its variant and workgroups per chunk ----
    row("xyzi_199_chunks", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, n_chunks=199, expect=dict(finish_threads=1024, finish_bpv=2, splits=4)),
    row("xyzi_200_chunks", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, n_chunks=200, expect=dict(finish_threads=512, finish_bpv=2, splits=2)),
    row("xyzi_511_chunks", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, n_chunks=511, expect=dict(finish_threads=512, splits=2)),
    row("xyzi_512_chunks", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, n_chunks=512, expect=dict(finish_threads=512, splits=1)),
    row("xyz_255_chunks", FUSED + FIN, **XYZ, fields=XYZ_F, n_chunks=255, expect=dict(finish_threads=256, finish_bpv=0, splits=16)),
    row("xyz_256_chunks", FUSED + FIN, **XYZ, fields=XYZ_F, n_chunks=256, expect=dict(finish_threads=256, splits=4)),
    row("xyz_1023_chunks", FUSED + FIN, **XYZ, fields=XYZ_F, n_chunks=1023, expect=dict(splits=4)),
    row("xyz_1024_chunks", FUSED + FIN, **XYZ, fields=XYZ_F, n_chunks=1024, expect=dict(splits=1)),
    row("xyzi_hint_palette", FUSED + SECS + FIN, **XYZI, fields=XYZI_F, hints=[0x2], data="few",
        expect=dict(probe="pieces", fused_field=0, runs=[], pal16=[], finish_threads=1024, finish_bpv=2)),
    row("xyzi_hint_runs", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, hints=[0xD], data="walk",
        expect=dict(probe="pieces", fused_field=-1, runs=[0], pal16=[], finish_threads=256, finish_bpv=0, splits=16)),
    row("xyz_u64_u16", FUSED + PROBE_FAST + RUNS + PAL64 + SECS + FIN, 32, xyz(), [(8, 16), (2, 24)], fields=XYZ_F + [(10, 16, 0), (4, 24, 0)],
        expect=dict(variant=variant(3, 8, 0, 3, 0), probe="fast", fused_field=1, runs=[1], pal16=[], pal64=[0], finish_threads=1024, finish_bpv=2)),
    row("xyz_2_u16_hints_d_f", FUSED + RUNS + SECS + FIN, 16, xyz(), [(2, 12), (2, 14)], hints=[0xD, 0xF], gpu=0,
        why="a hint is the union of the clouds' modes of an earlier call: 0xD and 0xF want clouds that differ (one cloud: xyz_2_u16_hints_1_2)",
        expect=dict(fused_field=1, runs=[0, 1], pal16=[])),
    row("xyz_2_u16_hints_1_2", FUSED + RUNS + SECS + FIN, 16, xyz(), [(2, 12), (2, 14)], fields=XYZI_F + [(4, 14, 0)], hints=[0x1, 0x2],
        data=["walk", "few"], expect=dict(fused_field=1, runs=[0], pal16=[], finish_threads=1024, finish_bpv=2)),
    row("xyz_u16_u32_u16", FUSED + RUNS + ["k_section_palette32"] * 2 + SECS + FIN, 20, xyz(), [(2, 12), (4, 14), (2, 18)],
        fields=XYZI_F + [(6, 14, 0), (4, 18, 0)],
        expect=dict(fused_field=0, runs=[0, 2, 1], pal16=[2], pal32=[1])),
    # ---- sub-chunks of the generic kernel, workgroups per chunk of the piece kernel ----
    row("2_floats_374_chunks", GENERIC + FIN, 8, TWO_FLOATS, fields=TWO_FLOATS_F, n_chunks=374, expect=dict(subs=32, sub_points=1024, sub_stride=20736)),
    row("2_floats_375_chunks", GENERIC + FIN, 8, TWO_FLOATS, fields=TWO_FLOATS_F, n_chunks=375,
        expect=dict(subs=16, sub_points=2048, sub_stride=41216, segs_per_chunk=16, reg_stride=16 * 41216, slot_stride=16 * 41216)),
    row("2_floats_5999_chunks", GENERIC + FIN, 8, TWO_FLOATS, n_chunks=5999, gpu=0, why="above 1024 chunks", expect=dict(subs=2)),
    row("2_floats_6000_chunks", GENERIC + FIN, 8, TWO_FLOATS, n_chunks=6000, gpu=0, why="above 1024 chunks", expect=dict(subs=1, sub_points=32768)),
    # ---- chunk-table output: one regular segment per chunk ----
    row("xyzi_table", FUSED + RUNS + PAL32 + SECS + ["k_chunk_sizes"], **XYZI, fields=XYZI_F, table=1,
        expect=dict(intra=1, subs=1, sub_points=504, sub_stride=4 * 7680 * 17, wave_stride=7680 * 17, piece_stride=7680, segs_per_chunk=3,
                    append=1, fused_field=-1, runs=[0], pal16=[0], close="chunk_sizes", kernel_clears=0, probe="pieces", writes_caller_modes=0)),
    row("xyz_2_u16_table", FUSED + RUNS + PAL32 + SECS + ["k_chunk_sizes"], 16, xyz(), [(2, 12), (2, 14)], fields=XYZI_F + [(4, 14, 0)], table=1,
        expect=dict(intra=1, subs=1, append=0, segs_per_chunk=5)),
    # ---- WIDE ----
    row("wide", ["k_wide_encode"] + FIN, 260, [], wide=1, max_regular_bytes=325, fields=[(7, 4 * k, 1) for k in range(65)],
        expect=dict(regular="wide", prepass="none", probe="none", subs=1, segs_per_chunk=1, finish_threads=256, finish_bpv=0, splits=16,
                    slot_stride=(32768 * 325 + 64 + 255) & ~255, kernel_clears=0)),
    row("wide_1_gorilla", ["k_gorilla_tokens", "k_wide_encode"] + FIN, 268, [], wide=1, wide_gorilla=1, max_regular_bytes=660,
        fields=[(8, 0, 0)] + [(7, 8 + 4 * k, 1) for k in range(65)],
        expect=dict(prepass="wide_groups", prepass_groups=1)),
    row("wide_64_gorilla", ["k_gorilla_tokens", "k_wide_encode"] + FIN, 520, [], wide=1, wide_gorilla=64, max_regular_bytes=660,
        fields=[(8, 8 * k, 0) for k in range(64)] + [(7, 512, 1), (7, 516, 1)],
        expect=dict(prepass_groups=1)),
    row("wide_65_gorilla", ["k_gorilla_tokens"] * 2 + ["k_wide_encode"] + FIN, 528, [], wide=1, wide_gorilla=65, max_regular_bytes=660,
        fields=[(8, 8 * k, 0) for k in range(65)] + [(7, 520, 1), (7, 524, 1)], expect=dict(prepass_groups=2)),
    row("wide_65_u16_table", ["k_wide_probe", "k_wide_encode", "k_chunk_sizes"], 142, [], wide=1, wide_adaptive=65, table=1, max_regular_bytes=15,
        fields=XYZ_F + [(4, 12 + 2 * k, 0) for k in range(65)],
        expect=dict(probe="wide", close="chunk_sizes", slot_stride=(32768 * (15 + 11 * 65) + 16 * 65 + 64 + 255) & ~255)),
    row("wide_65_u16_forced", ["k_wide_encode"] + FIN, 142, [], wide=1, wide_adaptive=65, forced=[0x1] * 65, max_regular_bytes=15,
        fields=XYZ_F + [(4, 12 + 2 * k, 0) for k in range(65)],
        expect=dict(probe="none")),
    # ---- no chunk ----
    row("xyzi_no_chunks", [], **XYZI, fields=XYZI_F, n_chunks=0,
        expect=dict(regular="none", close="offsets_memset", piece_pts=504, intra=0, kernel_clears=0, probe="none", sections=0)),
    row("xyzi_no_chunks_table", [], **XYZI, fields=XYZI_F, n_chunks=0, table=1, expect=dict(regular="none", close="none", intra=0)),
    row("wide_no_chunks", [], 260, [], wide=1, n_chunks=0, fields=[(7, 4 * k, 1) for k in range(65)], expect=dict(regular="none", close="offsets_memset")),
    # ---- kernel_clears: the headline shape has it (row xyzi); gone for each reason alone (table, Gorilla pre-pass, no chunk: above) ----
    row("xyzi_pipeline_1", GENERIC + PROBE_FAST + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, pipeline=1,
        expect=dict(regular="generic", variant=-1, piece_pts=0, kernel_clears=0, probe="fast", fused_field=0)),
    row("xyzi_pipeline_2", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, pipeline=2, expect=HEADLINE),
    row("xyzi_lz4", FUSED + RUNS + SECS + FIN, **XYZI, fields=XYZI_F, lz4=1, expect=dict(regular="pieces", kernel_clears=0, writes_caller_modes=0)),
    row("xyzi_new_zero_block", FUSED + RUNS + SECS + FIN, **XYZI, new_zero_block=1, gpu=0,
        why="no switch of the ABI: the first call of a codec (every traced row without hints is one); the kernels are those of xyzi", expect=dict(regular="pieces", kernel_clears=0)),
]


def abi_facts(r, host_input=False):
    """(EncodeFacts scalars, mode hints) as encode_stage1_once (hip_abi.hip) fills them for the row's plan and call."""
    c = r["call"]
    n_chunks = c.get("n_chunks", 2)
    n_clouds = c.get("n_clouds", 1)
    n_points = (n_chunks - n_clouds) * 32768 + 100 * n_clouds if n_chunks else 0  # every cloud ends with a chunk of 100 points
    na = c.get("wide_adaptive", 0) if c.get("wide") else len(r["adaptive"])
    forced = c.get("forced")
    hints = list(forced or c.get("hints") or []) + [0xF] * 64
    # the modes may go to the caller's array: device output, no LZ4 stage, no table, not forced (the rows are device-resident calls)
    caller_modes = int(not host_input and not c.get("lz4") and not c.get("table") and not forced)
    facts = [n_chunks, n_clouds, n_points, c.get("pipeline", 0), c.get("wide", 0), c.get("table", 0), c.get("lz4", 0),
             0 if host_input else c.get("residue", 0), int(bool(forced) and na > 0), caller_modes, int(not c.get("new_zero_block")),
             c.get("out_capacity", 1 << 62), na if c.get("wide") else 0, c.get("wide_gorilla", 0)]
    return facts, hints[:64]


def build_shim(folder):
    so = os.path.join(str(folder), "libencroute.so")
    # no HIP include path: the header and what it includes are plain C++
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"),
                    os.path.join(ROOT, "tests", "encode_route_shim.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    L.encode_route_of.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_uint32]
    L.encode_route_fused_variants.restype = C.c_uint32
    L.encode_route_section_stride.restype = C.c_uint32
    return L


def route_of(L, r, host_input=False):
    """(kernel names, scalar fields and section lists by name) of the row's route."""
    ops = [x for op in r["ops"] for x in op]
    ad = [x for a in r["adaptive"] for x in a]
    facts, hints = abi_facts(r, host_input)
    out = (C.c_int64 * len(FIELDS))()
    lists = (C.c_int32 * (4 * 65))()
    names = C.create_string_buffer(1024)
    n = L.encode_route_of(r["step"], len(r["ops"]), (C.c_uint32 * max(1, len(ops)))(*ops), len(r["adaptive"]), (C.c_uint32 * max(1, len(ad)))(*ad),
                          r["call"].get("max_regular_bytes", 0), (C.c_uint64 * len(facts))(*facts), (C.c_uint8 * 64)(*hints), out, lists, names,
                          len(names))
    assert n >= 0
    got = dict(zip(FIELDS, out))
    for key, table in (("regular", REGULAR), ("prepass", PREPASS), ("probe", PROBE), ("close", CLOSE)):
        assert 0 <= got[key] < len(table), (key, got[key])
        got[key] = table[got[key]]
    for l, key in enumerate(LISTS):
        got[key] = list(lists[65 * l + 1:65 * l + 1 + lists[65 * l]])
    kernels = names.value.decode().split()
    assert len(kernels) == n
    return kernels, got


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("route"))


def test_header_builds_alone(tmp_path):
    """No HIP call, no kernel header: a plain C++17 compiler takes the route header by itself, without a HIP include path."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "stage1_encode_route.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), str(src)],
                   check=True)


def test_tables(shim):
    assert shim.encode_route_fused_variants() == len(FUSED_VARIANTS) == 17
    assert shim.encode_route_section_stride() == SECTION_STRIDE


def test_row_names_are_unique():
    assert len({r["name"] for r in ROWS}) == len(ROWS)


def test_rows_are_traced_or_say_why_not():
    for r in ROWS:
        if r["call"].get("gpu", 1):
            assert r["fields"], r["name"]
        else:
            assert r["call"].get("why"), r["name"]


def test_every_fused_variant_has_a_row(shim):
    assert {route_of(shim, r)[1]["variant"] for r in ROWS} >= set(range(len(FUSED_VARIANTS)))


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_route(shim, r):
    kernels, got = route_of(shim, r)
    assert kernels == r["kernels"]
    for key, want in r["expect"].items():
        assert got[key] == want, (key, got[key], want)
    na = r["call"].get("wide_adaptive", 0) if r["call"].get("wide") else len(r["adaptive"])
    # every scalar is in range, and says nothing where it does not apply
    pieces = got["regular"] == "pieces"
    if got["variant"] >= 0:
        assert (got["lanes"], got["loadw"], got["unal"], got["l3"], got["tail"]) == FUSED_VARIANTS[got["variant"]]
        assert (got["tail_op"] >= 0) == bool(got["tail"]) and got["piece_pts"] == (504 if got["lanes"] == 3 else 378)
    else:
        assert not pieces and got["piece_pts"] == 0 and got["tail_op"] == -1
    assert (got["probe"] == "pieces") == (got["n_probe"] != 0) and got["writes_caller_modes"] <= (got["probe"] == "pieces")
    assert (got["pieces_lds"] != 0) == pieces and got["intra"] <= pieces and got["kernel_clears"] <= pieces
    assert (got["fixed_bytes"] != 0) == (got["regular"] in ("fixed", "fixed_direct"))
    assert (got["close"] == "finish") == (got["finish_threads"] > 0)
    if got["close"] == "finish":
        assert FINISH_VARIANTS[(got["finish_threads"], got["finish_bpv"])] == got["finish_lds"]
        assert (got["finish_bpv"] != 0) == (got["fused_field"] >= 0)
    assert got["fused_field"] not in got["pal16"] + got["pal32"] + got["pal64"]
    assert got["sections"] == (na != 0 and got["regular"] not in ("none", "wide", "fixed_direct"))
    if not got["sections"]:
        assert not (got["runs"] or got["pal16"] or got["pal32"] or got["pal64"] or got["append"] or got["sec_grid"])
    # the geometry the kernels share
    if pieces:
        assert got["sub_stride"] == 4 * got["piece_stride"] * (got["piece_wgs"] if got["intra"] else 1)
        assert got["wave_stride"] * 4 == got["sub_stride"] and got["subs"] == (1 if got["intra"] else got["piece_wgs"])
        assert got["slot_stride"] == got["reg_stride"] + na * SECTION_STRIDE
    if got["regular"] != "wide" and not r["call"].get("wide"):
        assert got["segs_per_chunk"] == got["subs"] + 2 * na and got["reg_stride"] == got["subs"] * got["sub_stride"]


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_staged_host_input_takes_the_aligned_route(shim, r):
    """Host input is staged into an aligned device buffer: its route is the one of an aligned device pointer (but for where the
    modes go: a host call has no device array for them)."""
    aligned = dict(r, call=dict(r["call"], residue=0))
    k_host, host = route_of(shim, r, host_input=True)
    k_dev, dev = route_of(shim, aligned)
    assert k_host == k_dev
    assert {k: v for k, v in host.items() if k != "writes_caller_modes"} == {k: v for k, v in dev.items() if k != "writes_caller_modes"}
    assert not host["writes_caller_modes"]


def design_table(L):
    """The encode route table of DESIGN.md section 4: one line per row, from encode_route() / encode_route_kernels()."""
    lines = ["| row | regular encoder | modes | sections | closing | slot geometry | kernels in launch order |", "|---|---|---|---|---|---|---|"]
    for r in ROWS:
        kernels, g = route_of(L, r)
        regular = g["regular"] if g["prepass"] == "none" else f"{g['prepass']} + {g['regular']}"
        if g["regular"] == "pieces":
            regular += f" <{g['lanes']}, {g['loadw']}, {'unal' if g['unal'] else 'al'}, l3 {g['l3']}" + (", tail" if g["tail"] else "") + ">"
            regular += ", intra" if g["intra"] else ""
            regular += ", clears" if g["kernel_clears"] else ""
        modes = g["probe"] + (f" (lds {g['pieces_lds']})" if g["probe"] == "pieces" else "")
        sections = " ".join(f"{k} {g[k]}" for k in LISTS if g[k]) or "--"
        sections += f", fused {g['fused_field']}" if g["fused_field"] >= 0 else ""
        sections += ", append" if g["append"] else ""
        closing = g["close"] + (f" <{g['finish_threads']}, {g['finish_bpv']}> x{g['splits']}" if g["close"] == "finish" else "")
        geometry = f"{g['subs']} x {g['sub_stride']}, {g['segs_per_chunk']} segs, slot {g['slot_stride']}"
        lines.append(f"| `{r['name']}` | {regular} | {modes} | {sections} | {closing} | {geometry} | {' '.join(kernels) or '--'} |")
    return lines


def test_design_md_holds_the_route_table(shim):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for line in design_table(shim):
        assert line in text, line
