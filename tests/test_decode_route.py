"""cloudini_amd/csrc/stage1_decode_route.h -- which kernels decode a batch -- compiled with g++ and checked against a table of
expected kernel sequences, on the CPU. The table was filled by reading the launcher the route replaced; tools/decode_route_trace.py
checks it against kernel traces of both (profiles/r13_a_decode_route_kernels.txt)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QF32, LF32, LF64, INT, COPY, XOR32, XOR64, GOR = range(8)  # DevOp::kind (stage1_device.h)
REGULAR = ("none", "wide", "points", "stream", "stream_cols", "fixed", "form", "stream_bitmap", "mixed_varint", "gorilla",
           "varint_tiles", "serial")
MARKER = ("none", "automaton32", "automaton64", "token_ends")
COLUMNS = ("none", "cols", "many")
REDO = ("none", "qf32", "any")
SECTIONS = ("none", "side_by_side", "small_general")
FIELDS = ("build_chunks", "lz4", "regular", "marker", "variant", "nops", "nf", "sm", "columns", "locate_waves", "scf", "section_dv",
          "scf_parts", "split_parts", "tail", "tail_sections", "redo", "redo_only", "sections", "general", "fast", "fast_sections",
          "fixed_bytes", "automaton_states")
POINTS_VARIANTS = {(3, 0, 1), (3, 1, 1), (3, 1, 2), (3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 8, 0), (4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 8, 0)}

BUILD, WALK = ["k_build_chunks"], ["k_walk_chunks"]
CHAINED = ["k_decode_points_w"]
SPLIT = ["k_wp_counts", "k_decode_points_w", "k_wp_carry", "k_decode_points_w"]
SIDE_COLS = ["k_locate_sections", "k_section_offsets", "k_sections_w", "k_sections_done"]  # launch_section_columns
SIDE_SECTIONS = ["k_section_offsets", "k_sections_w", "k_decode_stream_w", "k_sections_done", "k_decode_sections"]
SMALL_GENERAL = ["k_decode_sections_small", "k_decode_sections"]
TAIL, GENERAL, VARINT, STREAM = ["k_decode_tail"], ["k_decode_general"], ["k_decode_varint"], ["k_decode_stream_w"]
COLS_ALL = ["k_locate_sections", "k_section_dv_w", "k_sections_cols_fast", "k_decode_sections_cols"]
COLS_NO_DV = ["k_locate_sections", "k_sections_cols_fast", "k_decode_sections_cols"]
COLS_DV_ONLY = ["k_locate_sections", "k_section_dv_w", "k_decode_sections_cols"]
COLS_PLAIN = ["k_locate_sections", "k_decode_sections_cols"]


def xyz(first=0):
    return [(QF32, 4, first), (QF32, 4, first + 4), (QF32, 4, first + 8)]


def u16s(n, first=12):
    return [(2, first + 2 * a) for a in range(n)]


XYZ_U16 = dict(step=16, ops=xyz(), adaptive=[(2, 12)], v5=1)
# fields: what tools/decode_route_trace.py builds the same plan from through the C ABI: (type, offset, has resolution); the
# encoding is LOSSY unless `lossless`. data: how that script fills the integer fields (walk / few / runs).
XYZ_U16_FIELDS = [(7, 0, 1), (7, 4, 1), (7, 8, 1), (4, 12, 0)]


def row(name, kernels, step, ops, adaptive=(), v5=0, fields=None, expect=None, **call):
    return dict(name=name, kernels=kernels, step=step, ops=list(ops), adaptive=list(adaptive), v5=v5, fields=fields, expect=expect or {},
                call=call)


# call: n_chunks (2), sized (1), lz4, fill_zero, aligned (1), palette_hint, dv_hint, force_parts (the test hook), and facts the
# ABI never produces: no_cols, no_dsec, max_regular_bytes. gpu=0: not reachable through the ABI, the trace script skips the row.
ROWS = [
    row("xyz", BUILD + SPLIT + TAIL, 12, xyz(), fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1)],
        expect=dict(regular="points", nops=3, nf=0, sm=1, split_parts=16, columns="none", tail=1, tail_sections=0, general=0)),
    row("xyz_100_chunks", BUILD + CHAINED + TAIL, 12, xyz(), n_chunks=100, gpu=0,
        expect=dict(nops=3, nf=0, sm=1, split_parts=1, tail_sections=0)),
    row("xyz_u16_100_chunks", BUILD + COLS_ALL + CHAINED + TAIL, **XYZ_U16, n_chunks=100, fill_zero=1, gpu=0,
        expect=dict(nops=3, nf=1, sm=2, split_parts=1, locate_waves=4, scf_parts=6, section_dv=1, tail_sections=1)),
    row("xyz_u16_fill_zero", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, fill_zero=1,
        expect=dict(nops=3, nf=1, sm=2, columns="cols", scf=1, locate_waves=16, scf_parts=16, split_parts=16, tail_sections=1)),
    row("xyz_u16_fill_zero_unaligned_out", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, fill_zero=1, aligned=0,
        expect=dict(nf=1, sm=1)),
    row("xyz_u16", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, expect=dict(nops=3, nf=1, sm=1)),
    row("xyz_u16_odd_offset", BUILD + COLS_ALL + SPLIT + TAIL, 16, xyz(), [(2, 13)], v5=1, fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1), (4, 13, 0)],
        expect=dict(nops=3, nf=1, sm=0)),
    row("xyz_u16_palette_hint", BUILD + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, fill_zero=1, palette_hint=1, dv_hint=1, data="few",
        expect=dict(nf=1, sm=2, columns="none", tail_sections=1)),
    row("xyz_u16_dv_hint_1", BUILD + COLS_NO_DV + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, fill_zero=1, dv_hint=1, data="runs",
        expect=dict(nf=1, sm=2, section_dv=0, scf_parts=16)),
    row("xyz_u16_dv_hint_2", BUILD + COLS_DV_ONLY + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, fill_zero=1, dv_hint=2, data="walk",
        expect=dict(nf=1, sm=2, section_dv=1, scf_parts=0, scf=1)),
    row("xyz_u16_no_cols", BUILD + SPLIT + TAIL, **XYZ_U16, fill_zero=1, no_cols=1, gpu=0, expect=dict(nf=1, sm=2, columns="none")),
    row("xyz_u16_1_chunk", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, n_chunks=1, gpu=0,
        expect=dict(split_parts=16, locate_waves=16, scf_parts=16)),
    row("xyz_u16_64_chunks", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, n_chunks=64, gpu=0,
        expect=dict(split_parts=4, locate_waves=16, scf_parts=8)),
    row("xyz_u16_65_chunks", BUILD + COLS_ALL + CHAINED + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, n_chunks=65,
        expect=dict(split_parts=1, locate_waves=4, scf_parts=8)),
    row("xyz_u16_600_chunks", BUILD + COLS_ALL + CHAINED + TAIL, **XYZ_U16, n_chunks=600, gpu=0,
        expect=dict(split_parts=1, locate_waves=4, scf_parts=1)),
    row("xyz_u16_parts_1", BUILD + COLS_ALL + CHAINED + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, force_parts=1, expect=dict(split_parts=1)),
    row("xyz_u16_parts_3", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, fields=XYZ_U16_FIELDS, force_parts=3, expect=dict(split_parts=3)),
    row("xyz_u16_65_chunks_parts_3", BUILD + COLS_ALL + SPLIT + TAIL, **XYZ_U16, n_chunks=65, force_parts=3, gpu=0,
        expect=dict(split_parts=3, locate_waves=4)),
    row("xyz_2_u16", BUILD + COLS_PLAIN + SPLIT + TAIL, 16, xyz(), u16s(2), v5=1, fields=XYZ_U16_FIELDS + [(4, 14, 0)],
        expect=dict(nops=3, nf=2, sm=0, columns="cols", scf=0, section_dv=0, scf_parts=0, tail_sections=1)),
    row("xyz_5_ints", BUILD + SIDE_COLS + SPLIT + VARINT + SMALL_GENERAL + GENERAL, 28, xyz(), u16s(2) + [(4, 16), (4, 20), (4, 24)], v5=1,
        fields=XYZ_U16_FIELDS + [(4, 14, 0), (6, 16, 0), (6, 20, 0), (6, 24, 0)],
        expect=dict(nops=3, nf=8, sm=0, columns="many", tail=0, redo="qf32", redo_only=1, sections="small_general", fast=1, fast_sections=1)),
    row("xyz_5_ints_one_u64", BUILD + SPLIT + VARINT + SMALL_GENERAL + GENERAL, 28, xyz(), u16s(4) + [(8, 20)], v5=1,
        fields=XYZ_U16_FIELDS + [(4, 14, 0), (4, 16, 0), (4, 18, 0), (10, 20, 0)],
        expect=dict(nops=3, nf=0, sm=1, columns="none", tail=0, sections="small_general")),
    row("xyz_5_ints_no_cols", BUILD + SPLIT + VARINT + SIDE_SECTIONS + GENERAL, 28, xyz(), u16s(2) + [(4, 16), (4, 20), (4, 24)], v5=1,
        no_cols=1, gpu=0, expect=dict(nf=0, sm=1, columns="none", sections="side_by_side")),
    row("xyz_9_u16", BUILD + SPLIT + VARINT + SMALL_GENERAL + GENERAL, 30, xyz(), u16s(9), v5=1,
        fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1)] + [(4, 12 + 2 * a, 0) for a in range(9)],
        expect=dict(nops=3, nf=0, sm=0, columns="none", sections="small_general")),
    row("xyzw", BUILD + SPLIT + TAIL, 16, xyz() + [(QF32, 4, 12)], fields=[(7, 4 * k, 1) for k in range(4)],
        expect=dict(regular="points", nops=4, nf=0, sm=0, tail_sections=0)),
    row("xyzw_u16", BUILD + COLS_ALL + SPLIT + TAIL, 20, xyz() + [(QF32, 4, 12)], [(2, 16)], v5=1, gpu=0, expect=dict(nops=4, nf=1, sm=0)),
    row("2_floats_u16", BUILD + SIDE_COLS + STREAM + VARINT + SMALL_GENERAL + GENERAL, 12, [(LF32, 4, 0), (LF32, 4, 4)], [(2, 8)], v5=1,
        fields=[(7, 0, 1), (7, 4, 1), (4, 8, 0)],
        expect=dict(regular="stream_cols", redo="any", redo_only=1, sections="small_general", fast=1, fast_sections=1)),
    row("2_floats_u16_no_dsec", BUILD + STREAM + VARINT + SMALL_GENERAL + GENERAL, 12, [(LF32, 4, 0), (LF32, 4, 4)], [(2, 8)], v5=1, no_dsec=1,
        gpu=0, expect=dict(regular="stream", redo="any", redo_only=1, sections="small_general")),
    row("2_floats_u16_no_cols", BUILD + STREAM + VARINT + SIDE_SECTIONS + GENERAL, 12, [(LF32, 4, 0), (LF32, 4, 4)], [(2, 8)], v5=1, no_cols=1,
        gpu=0, expect=dict(regular="stream", sections="side_by_side")),
    row("2_floats", BUILD + STREAM + VARINT + GENERAL, 8, [(LF32, 4, 0), (LF32, 4, 4)], fields=[(7, 0, 1), (7, 4, 1)],
        expect=dict(regular="stream", redo="any", redo_only=1, sections="none", fast=1, fast_sections=0)),
    # more than 8 varint ops: no parallel kernel takes the stream
    row("9_floats", BUILD + GENERAL, 36, [(LF32, 4, 4 * k) for k in range(9)], fields=[(7, 4 * k, 1) for k in range(9)],
        expect=dict(regular="serial", redo="none", fast=0)),
    # k_decode_varint<8, true> alone: 8 varint ops whose point may exceed kSwMaxPointBytes (no plan of the ABI has such a point)
    row("8_floats_long_points", BUILD + VARINT + GENERAL, 32, [(LF32, 4, 4 * k) for k in range(8)], max_regular_bytes=100, gpu=0,
        expect=dict(regular="varint_tiles", redo="any", redo_only=0, fast=1)),
    row("xyz_raw4", BUILD + ["k_mark_ends_automaton"] + STREAM + GENERAL, 16, xyz() + [(COPY, 4, 12)],
        fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1), (7, 12, 0)],
        expect=dict(regular="stream_bitmap", marker="automaton32", automaton_states=7, redo="none", fast=1, sections="none")),
    row("xyz_raw8", BUILD + ["k_mark_ends_automaton"] + STREAM + GENERAL, 20, xyz() + [(XOR64, 8, 12)], gpu=0,
        expect=dict(regular="stream_bitmap", marker="automaton64", automaton_states=11)),
    row("xyz_2_raw4", BUILD + ["k_mark_ends_automaton"] + STREAM + GENERAL, 20, xyz() + [(COPY, 4, 12), (COPY, 4, 16)],
        fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1), (7, 12, 0), (7, 16, 0)],
        expect=dict(regular="stream_bitmap", marker="automaton64", automaton_states=11)),
    row("xyz_4_raw4_form", BUILD + STREAM + GENERAL, 28, xyz() + [(COPY, 4, 12 + 4 * k) for k in range(4)],
        fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1)] + [(7, 12 + 4 * k, 0) for k in range(4)],
        expect=dict(regular="form", marker="none", automaton_states=0, fast=1)),
    # a form beyond kSwMaxPointBytes (no plan of the ABI has one: 8 ops of at most 10 bytes)
    row("xyz_raw4_long_points", BUILD + ["k_mark_token_ends"] + VARINT + GENERAL, 16, xyz() + [(COPY, 4, 12)], max_regular_bytes=100, gpu=0,
        expect=dict(regular="mixed_varint", marker="token_ends", redo="none", fast=1)),
    row("4_raw", BUILD + ["k_decode_fixed"] + GENERAL, 16, [(XOR32, 4, 4 * k) for k in range(4)], fields=[(7, 4 * k, 0) for k in range(4)],
        lossless=1, expect=dict(regular="fixed", marker="none", fixed_bytes=16, fast=1)),
    row("8_raw", BUILD + ["k_decode_fixed"] + GENERAL, 32, [(XOR32, 4, 4 * k) for k in range(8)], gpu=0, expect=dict(regular="fixed", fixed_bytes=32)),
    row("9_raw", BUILD + GENERAL, 36, [(XOR32, 4, 4 * k) for k in range(9)], fields=[(7, 4 * k, 0) for k in range(9)], lossless=1,
        expect=dict(regular="serial", marker="none", fast=0)),
    row("xyz_gorilla", BUILD + STREAM + GENERAL, 20, xyz() + [(GOR, 8, 12)], fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1), (8, 12, 0)],
        expect=dict(regular="gorilla", redo="none", fast=1)),
    row("2_gorilla_odd_raw", BUILD + GENERAL, 24, [(GOR, 8, 0), (GOR, 8, 8), (LF32, 4, 16), (COPY, 3, 20)], gpu=0,
        expect=dict(regular="serial", fast=0)),
    row("2_gorilla_7_floats", BUILD + GENERAL, 44, [(LF32, 4, 4 * k) for k in range(7)] + [(GOR, 8, 28), (GOR, 8, 36)],
        fields=[(7, 4 * k, 1) for k in range(7)] + [(8, 28, 0), (8, 36, 0)], expect=dict(regular="serial", fast=0)),
    row("xyz_gorilla_u16", BUILD + STREAM + SIDE_SECTIONS + GENERAL, 22, xyz() + [(GOR, 8, 12)], [(2, 20)], v5=1,
        fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1), (8, 12, 0), (4, 20, 0)], expect=dict(regular="gorilla", sections="side_by_side", fast_sections=1)),
    row("wide", BUILD + ["k_decode_wide"], 260, [], wide=1, fields=[(7, 4 * k, 1) for k in range(65)], expect=dict(regular="wide", general=0, tail=0)),
    row("xyz_lz4", WALK + ["k_lz4_decode_chunks"] + SPLIT + TAIL, 12, xyz(), fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1)], lz4=1, sized=0,
        expect=dict(lz4=1, build_chunks=0)),
    row("xyz_unsized", WALK + SPLIT + TAIL, 12, xyz(), fields=[(7, 0, 1), (7, 4, 1), (7, 8, 1)], sized=0, expect=dict(lz4=0, build_chunks=0)),
    row("xyz_no_chunks", BUILD, 12, xyz(), n_chunks=0, gpu=0, expect=dict(regular="none", general=0)),
]


def varint_and_raw(ops):
    """DevPlan::varint_and_raw as cldn_hip_plan_create sets it."""
    raw = [k in (COPY, XOR32, XOR64) for k, _, _ in ops]
    ok = 1 <= len(ops) <= 8 and sum(s if r else (5 if k == QF32 else 10) for (k, s, _), r in zip(ops, raw)) <= 256
    ok = ok and all((s in (1, 2, 4, 8)) if r else k in (QF32, LF32, LF64, INT) for (k, s, _), r in zip(ops, raw))
    return bool(ok and any(raw))


def abi_facts(r, split_parts_of):
    """DecodeFacts as decode_framed (hip_abi.hip) fills the DecodeLaunch for the row's plan and call."""
    c = r["call"]
    n_chunks, na, v5, wide = c.get("n_chunks", 2), len(r["adaptive"]), r["v5"], c.get("wide", 0)
    dec_cols = bool(v5 and 1 <= na <= 8)
    cols = sum(1 << a for a, (bpv, _) in enumerate(r["adaptive"]) if dec_cols and bpv <= 4)
    wp_parts = c.get("force_parts") or split_parts_of(n_chunks)
    return [n_chunks, wp_parts, c.get("palette_hint", 0), c.get("dv_hint", 0), v5, wide, c.get("lz4", 0), c.get("sized", 1),
            c.get("fill_zero", 0), c.get("aligned", 1), 0 if c.get("no_cols") else cols,
            int(dec_cols and n_chunks > 0 and not c.get("no_dsec")), 1, 1, 1, int(dec_cols and na == 1 and n_chunks > 0),
            int(varint_and_raw(r["ops"]) and n_chunks > 0), int(not wide and wp_parts > 1)]


def build_shim(folder):
    from cloudini_amd import build as _build
    so = os.path.join(str(folder), "libdecroute.so")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build.HIPCC))), "include")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), os.path.join(ROOT, "tests", "decode_route_shim.cpp"), "-o", so],
                   check=True)
    L = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    L.route_of.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32, u32p, C.POINTER(C.c_int32), C.c_char_p, C.c_uint32]
    L.route_wp_split_parts.argtypes = [C.c_uint32]
    L.route_wp_split_parts.restype = C.c_uint32
    L.route_points_variants.restype = C.c_uint32
    return L


def route_of(L, r):
    """(kernel names, scalar fields by name) of the row's route."""
    ops = [x for op in r["ops"] for x in op]
    ad = [x for a in r["adaptive"] for x in a]
    facts = abi_facts(r, L.route_wp_split_parts)
    out = (C.c_int32 * len(FIELDS))()
    names = C.create_string_buffer(1024)
    n = L.route_of(r["step"], len(r["ops"]), (C.c_uint32 * max(1, len(ops)))(*ops), len(r["adaptive"]), (C.c_uint32 * max(1, len(ad)))(*ad),
                   r["call"].get("max_regular_bytes", 0), (C.c_uint32 * len(facts))(*facts), out, names, len(names))
    assert n >= 0
    got = dict(zip(FIELDS, out))
    for key, table in (("regular", REGULAR), ("marker", MARKER), ("columns", COLUMNS), ("redo", REDO), ("sections", SECTIONS)):
        assert 0 <= got[key] < len(table), (key, got[key])
        got[key] = table[got[key]]
    kernels = names.value.decode().split()
    assert len(kernels) == n
    return kernels, got


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("route"))


def test_split_parts(shim):
    assert [shim.route_wp_split_parts(n) for n in (0, 1, 16, 17, 64, 65, 100, 128, 129, 600)] == [1, 16, 16, 15, 4, 1, 1, 1, 1, 1]
    assert shim.route_points_variants() == len(POINTS_VARIANTS)


def test_row_names_are_unique():
    assert len({r["name"] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_route(shim, r):
    kernels, got = route_of(shim, r)
    assert kernels == r["kernels"]
    for key, want in r["expect"].items():
        assert got[key] == want, (key, got[key], want)
    # every scalar is in range, and says nothing where it does not apply
    points = got["regular"] == "points"
    assert (got["variant"] >= 0) == points
    if points:
        assert (got["nops"], got["nf"], got["sm"]) in POINTS_VARIANTS
        assert 1 <= got["split_parts"] <= 16
        assert got["tail"] + got["general"] == 1 and got["tail_sections"] <= got["tail"]
    else:
        assert got["columns"] == "none" and got["split_parts"] == 1 and not got["tail"]
    if got["columns"] == "cols":
        assert got["locate_waves"] in (4, 16) and 0 <= got["scf_parts"] <= 16
        assert got["scf"] or not (got["section_dv"] or got["scf_parts"])
    else:
        assert not (got["locate_waves"] or got["scf"] or got["section_dv"] or got["scf_parts"])
    assert (got["marker"] != "none") <= (got["regular"] in ("stream_bitmap", "mixed_varint"))
    assert (got["fixed_bytes"] != 0) == (got["regular"] == "fixed")
    assert (got["sections"] != "none") == bool(got["fast_sections"]) and got["fast_sections"] <= got["fast"]
    assert got["redo_only"] <= (got["redo"] != "none")
    assert got["general"] == (got["regular"] not in ("none", "wide") and not got["tail"])


def design_table(L):
    """The route table of DESIGN.md section 4: one line per row, from decode_route() / decode_route_kernels()."""
    lines = ["| row | regular decoder | columns | behind it | kernels in launch order |", "|---|---|---|---|---|"]
    for r in ROWS:
        kernels, g = route_of(L, r)
        regular = g["regular"] if g["marker"] == "none" else f"{g['marker']} + {g['regular']}"
        if g["regular"] == "points":
            regular += f" <{g['nops']}, {g['nf']}, sm {g['sm']}>, " + (f"split x{g['split_parts']}" if g["split_parts"] > 1 else "chained")
        columns = g["columns"]
        if columns == "cols":
            columns += f" (locate<{g['locate_waves']}>" + (", dv" if g["section_dv"] else "") + (f", fast x{g['scf_parts']}" if g["scf_parts"] else "") + ")"
        if g["regular"] == "stream_cols":
            columns = "many"
        behind = ["tail" + (" + sections" if g["tail_sections"] else "")] if g["tail"] else []
        behind += [f"redo {g['redo']}"] if g["redo"] != "none" else []
        behind += [g["sections"]] if g["sections"] != "none" else []
        behind += ["general"] if g["general"] else []
        lines.append(f"| `{r['name']}` | {regular} | {columns} | {', '.join(behind) or '--'} | {' '.join(kernels)} |")
    return lines


def test_design_md_holds_the_route_table(shim):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for line in design_table(shim):
        assert line in text, line

