"""CPU: the value grid of tests/value_grid_cases.py is what it says. Every mark of every case holds in the numpy model (the row is in
the tier its name says, the token has the tick, reference and length its name says); the model's token lengths are the lengths of
the tokens the oracle wrote; the oracle's bytes are the compiled reference's, for every cloud and every hand-written stream; and the
totals the grid is built to reach are counted here, not stated in prose. tests/test_gpu_value_grid.py runs the grid on the device."""
import numpy as np
import pytest

import sweep_model as SM
import value_grid_cases as V

FILL = 0x5A
GROUP_IDS = [V.group_id(g) for g in V.GROUPS]
E_CASES = V.e_cases()


def _chunks(stream):
    s, pos, out = np.asarray(stream, dtype=np.uint8), 0, []
    while pos < len(s):
        size = int.from_bytes(s[pos:pos + 4].tobytes(), "little")
        out.append(s[pos + 4:pos + 4 + size])
        pos += 4 + size
    return out


@pytest.mark.parametrize("group", V.GROUPS, ids=GROUP_IDS)
def test_every_mark_holds_in_the_model(group):
    cs = V.family(*group)
    assert cs
    for c in cs:
        assert c.marks, c.name
        assert c.n <= 70_000
        failed = c.pred()
        assert not failed, (c.name, failed[:5])


@pytest.mark.parametrize("group", V.GROUPS, ids=GROUP_IDS)
def test_the_model_has_the_oracles_token_lengths(oracle, group):
    """Layouts whose payload is nothing but varint tokens: every byte with a clear MSB ends a token, so the oracle's token lengths can
    be read off its bytes; they are the model's, token for token. The two layouts with other bytes: the size of the regular stream."""
    fam, layout = group
    for c in V.family(fam, layout):
        m = V.Model(c)
        stream = oracle.encode_stage1(c.info(), c.cloud())
        chunks = _chunks(stream)
        assert len(chunks) == (c.n + V.CHUNK - 1) // V.CHUNK
        want = np.stack([ln[3] for ln in m.lanes], axis=1)                    # [n, lanes]
        if layout == "COPY_F_COPY":
            assert sum(len(p) for p in chunks) == m.regular_bytes() + 8 * c.n, c.name
        else:
            assert layout != "XYZ_U16_F32" or sum(len(p) for p in chunks) > m.regular_bytes(), c.name
            at = 0
            for p in chunks:
                k = min(V.CHUNK, c.n - at)
                got = np.diff(np.nonzero(p < 0x80)[0], prepend=-1)
                if layout == "XYZ_U16_F32":      # the regular stream comes first, the integer field's section behind it
                    got = got[:k * want.shape[1]]
                assert np.array_equal(got, want[at:at + k].reshape(-1)), c.name
                at += k


@pytest.mark.parametrize("group", V.GROUPS, ids=GROUP_IDS)
def test_the_reference_writes_and_reads_the_same_bytes(oracle, reflib, group):
    for c in V.family(*group):
        info, cloud = c.info(), c.cloud()
        stream = oracle.encode_stage1(info, cloud)
        assert np.array_equal(reflib.encode_stage1(info, cloud), stream), c.name
        assert np.array_equal(reflib.decode_noheader(info, stream, fill=FILL), oracle.decode_stage1(info, stream, c.n, fill=FILL)), c.name


@pytest.mark.parametrize("case", E_CASES, ids=[e.name for e in E_CASES])
def test_the_reference_reads_the_hand_written_streams_as_the_oracle_does(oracle, reflib, case):
    info = case.info()
    want = oracle.decode_stage1(info, case.stream(oracle), case.n, fill=FILL)
    assert np.array_equal(reflib.decode_noheader(info, case.stream(oracle), fill=FILL), want)
    # the stream is what the writer says: the decoded ticks at resolution 1.0 are the running ticks, rounded once
    if case.res == 1.0:
        kinds = V.kinds_of(case.layout)
        cur = [0] * len(kinds)
        lanes = [f for f in V.LAYOUTS[case.layout][0] if f[3]]
        step = V.LAYOUTS[case.layout][1]
        for i, row in enumerate(case.points):
            for k, d in enumerate(row):
                dt = "<f8" if kinds[k] == SM.SCALAR64 else "<f4"
                got = want[i * step + lanes[k][1]:i * step + lanes[k][1] + np.dtype(dt).itemsize].view(dt)[0]
                if d is None:
                    cur[k] = 0
                    assert np.isnan(got)
                    continue
                cur[k] += d
                if kinds[k] == SM.FLOATN:
                    cur[k] = (cur[k] + (1 << 31)) % (1 << 32) - (1 << 31)
                assert got == np.array(cur[k], dtype=np.int64).astype(dt), (i, k, cur[k])      # int64 -> float: ONE rounding, to nearest even


# ---------------------------------------------------------------------------------------------------- totals over the grid
def _tags(fam, layouts=None):
    out = []
    for f, layout in V.GROUPS:
        if f == fam and (layouts is None or layout in layouts):
            for c in V.family(f, layout):
                m = V.Model(c)
                out += [(layout, k.tag) for k in c.marks if k.tag is not None and k.holds(m)]
    return out


def test_every_tier_length_and_sign_is_reached():
    """(tier, token length 1..4, sign of the delta) in the fast tier, the NaN tier and the integer formulas, plus 5 bytes in the latter;
    per layout of the piece kernel (4 lanes: no NaN tier)"""
    got = set(_tags("B"))
    for layout in V.PIECE_LAYOUTS:
        tiers = ("fast", "nan", "hard") if V.n_floatn(layout) == 3 else ("fast", "hard")
        want = {(layout, ("len", t, L, s)) for t in tiers for L in (1, 2, 3, 4) for s in (1, -1)} | {(layout, ("len", "hard", 5, s)) for s in (1, -1)}
        assert want <= got, sorted(want - got)
    # both sides of every 7-bit threshold: u = 2^(7L) - 1 and 2^(7L), L = 1..4 (u = 2^28 is a 5-byte token)
    for d in V.b_deltas(True):
        u = ((d[0] << 1) ^ (d[0] >> 63)) + 1
        assert V.zz1_len(d[0]) == (u.bit_length() + 6) // 7
    us = {((d << 1) ^ (d >> 63)) + 1 for d, _a, _b in V.b_deltas(True)}
    assert {(1 << (7 * L)) + e for L in (1, 2, 3, 4) for e in (-1, 0, 1)} <= us
    assert max(abs(x) for _d, a, b in V.b_deltas(False) for x in (a, b)) < V.LIMIT


def test_every_switch_tick_is_reached_at_every_index_in_every_lane():
    got = set(_tags("A"))
    for layout in V.PIECE_LAYOUTS:
        for T in V.A_TICKS:
            for lane in range(V.n_floatn(layout)):
                for i in V.A_INDEXES:
                    assert (layout, ("own", T, i, lane)) in got, (layout, T, i, lane)
                    assert i == 0 or (layout, ("front", T, i, lane)) in got, (layout, T, i, lane)
        assert {(layout, ("alt", T)) for T in (V.LIMIT - 1, V.LIMIT, 2 * V.LIMIT - 1)} <= got
        assert layout in V.TAIL_LAYOUTS or (layout, ("ovf", V.LIMIT - 1)) in got
    assert sorted(abs(t) for t in V.A_TICKS) == sorted(2 * [2097150, 2097151, 2097152, 2097153, 4194303])


def test_every_tier_is_reached_in_every_piece_layout():
    for layout in V.PIECE_LAYOUTS:
        seen = set()
        for fam in V.ENCODE_FAMILIES:
            for c in V.family(fam, layout):
                seen |= set(np.unique(V.Model(c).tier).tolist())
        want = {"fast", "hard"} | ({"nan"} if V.n_floatn(layout) == 3 else set()) | (set() if layout in V.TAIL_LAYOUTS else {"ovf"})
        assert seen == want, (layout, seen)


def test_rounding_and_range_rows_are_in_every_layout():
    for layout in V.LAYOUTS:
        kinds = set(V.kinds_of(layout))
        tags = {t for _l, t in _tags("C", (layout,))} | {t for _l, t in _tags("D", (layout,))}
        for kind in kinds:
            assert {("tie", kind), ("edge", kind), ("after_zero", kind), ("odd", kind)} <= tags, (layout, kind)
            assert sum(1 for t in tags if t[0] == "range" and t[1] == kind) == 20, (layout, kind)
        if SM.FLOATN in kinds:
            assert {("f32tie", 0.001), ("f32tie", 0.37)} <= tags, layout
    for res in (0.001, 0.37):                      # the finder has members at both resolutions
        v, t = V.VG.float32_only_ties(res, 20000)
        assert len(v) >= 80 and np.all(t - np.floor(t) == 0.5)
        exact = v.astype(np.float64) * float(np.float32(1) / np.float32(res))
        assert np.all(exact != t)


def test_every_stream_tick_is_reached_in_both_marker_states():
    for layout in V.E_LAYOUTS:
        kinds = V.kinds_of(layout)
        for res in V.E_RESOLUTIONS:
            es = [e for e in E_CASES if e.layout == layout and e.res == res and not e.long_tokens]
            reached = set().union(*[e.reached for e in es])
            wraps = set().union(*[e.wraps for e in es])
            for k, kind in enumerate(kinds):
                for T in (V.E_TICKS32 if kind == SM.FLOATN else V.E_TICKS32 + V.E_TICKS64):
                    assert (T, k, 0) in reached and (T, k, 1) in reached, (layout, res, T, k)
                if kind == SM.FLOATN:
                    assert (k, 0) in wraps and (k, 1) in wraps
    # the point decoder's two forms (stage1_decode_wave.h: with and without a marker in the piece of 992 payload bytes): the first ticks
    # lie more than two pieces in front of the first marker; around the second ticks every point carries a marker for more than a piece
    for e in E_CASES:
        if e.layout not in V.POINT_DECODER_LAYOUTS:
            continue
        size = np.array([sum(len(V.token(d)) for d in row) for row in e.points])
        start = np.concatenate([[0], np.cumsum(size)])
        marked = np.array([any(d is None for d in row) for row in e.points])
        assert not marked[:e.marked_from].any() and marked[e.marked_from:].all()
        # no token over 4 bytes, no 0x00 that ends a longer token: what the point kernel keeps (points_token_cases.plain)
        toks = [V.token(d) for row in e.points for d in row]
        assert max(len(t) for t in toks) == (5 if e.long_tokens else 4) and all(t[-1] != 0 or len(t) == 1 for t in toks), e.name
        assert start[e.marked_from] - start[max(e.tick_points[0]) + 1] > 2 * 992
        assert start[min(e.tick_points[1])] - start[e.marked_from] > 992 + 16 and start[-1] - start[max(e.tick_points[1]) + 1] > 992 + 16
    ticks = set(V.E_TICKS32 + V.E_TICKS64)
    assert {(1 << 24) + 1, -(1 << 25) - 6, (1 << 31) - 1, -(1 << 31), (1 << 62) + (1 << 38) + 1, (1 << 63) - 1, (1 << 53) + 3} <= ticks
    # the double-rounding trap: through double the tick rounds to 2^62, converted directly to 2^62 + 2^39
    t = (1 << 62) + (1 << 38) + 1
    assert float(np.float32(np.float64(t))) == float(1 << 62) and float(np.float32(np.int64(t))) == float((1 << 62) + (1 << 39))


# ---------------------------------------------------------------------------------------------------- the site a layout reaches
def _route_row(layout, res=0.5):
    """The layout as a row of tests/test_encode_route.py / tests/test_decode_route.py: ops (DevOp kind, size, offset), adaptive fields"""
    import test_decode_route as DR
    kind_of = {SM.FLOATN: DR.QF32, SM.SCALAR32: DR.LF32, SM.SCALAR64: DR.LF64}
    kinds = iter(V.kinds_of(layout))
    ops, adaptive = [], []
    for _nm, off, t, lossy in V.LAYOUTS[layout][0]:
        if lossy:
            ops.append((kind_of[next(kinds)], 8 if t == V.F.FLOAT64 else 4, off))
        elif t == V.F.FLOAT32:
            ops.append((DR.COPY, 4, off))
        else:
            adaptive.append((2, off))
    wide = layout == "WIDE"
    call = dict(wide=1, max_regular_bytes=sum(5 if k == DR.QF32 else 10 for k, _s, _o in ops)) if wide else {}
    return dict(name=layout, step=V.LAYOUTS[layout][1], ops=[] if wide else ops, adaptive=adaptive, v5=int(bool(adaptive)), call=call)


# layout -> (regular encoder, lanes, unal, l3, tail) and (regular decoder, marker kernel, redo behind it)
ENCODE_SITE = {"XYZ": ("pieces", 3, 0, 3, 0), "XYZI4": ("pieces", 4, 0, 3, 0), "XYZ_PAD_I": ("pieces", 4, 0, 4, 0), "XYZ_UNAL": ("pieces", 3, 1, 3, 0),
               "XYZ_F64": ("pieces", 3, 0, 3, 1), "XYZ_U16_F32": ("pieces", 3, 1, 3, 1), "FIVE": ("generic",), "LONE32": ("generic",),
               "LONE64": ("generic",), "COPY_F_COPY": ("generic",), "WIDE": ("wide",)}
DECODE_SITE = {"XYZ": ("points", "none", "none"), "XYZI4": ("points", "none", "none"), "XYZ_PAD_I": ("points", "none", "none"),
               "XYZ_UNAL": ("points", "none", "none"), "XYZ_F64": ("stream", "none", "any"), "XYZ_U16_F32": ("stream_cols", "none", "any"),
               "FIVE": ("stream", "none", "any"), "LONE32": ("stream", "none", "any"), "LONE64": ("stream", "none", "any"),
               "COPY_F_COPY": ("stream_bitmap", "automaton64", "none"), "WIDE": ("wide", "none", "none")}


@pytest.mark.parametrize("layout", V.LAYOUTS)
def test_the_layout_reaches_the_sites_it_is_named_for(layout, tmp_path_factory):
    """The route functions the launchers call (stage1_encode_route.h, stage1_decode_route.h), compiled as tests/test_encode_route.py
    and tests/test_decode_route.py compile them, on the layout's plan: the encoder and its instantiation, the regular decoder."""
    import test_decode_route as DR
    import test_encode_route as ER
    r = _route_row(layout)
    kernels, got = ER.route_of(_shim(tmp_path_factory, ER), r, host_input=True)
    want = ENCODE_SITE[layout]
    assert got["regular"] == want[0], got["regular"]
    if want[0] == "pieces":
        assert kernels[0] == "k_encode_fused" and got["variant"] >= 0
        assert (got["lanes"], got["unal"], got["l3"], got["tail"]) == want[1:], (got["lanes"], got["loadw"], got["unal"], got["l3"], got["tail"])
        assert ER.FUSED_VARIANTS[got["variant"]] == (got["lanes"], got["loadw"], got["unal"], got["l3"], got["tail"])
        if got["tail"]:
            assert got["tail_op"] == 3                  # the op behind the three FloatN lanes
    elif want[0] == "generic":
        assert kernels[0] == "k_encode_regular" and got["variant"] == -1
    else:
        assert kernels[0] == "k_wide_encode"
    kernels, got = DR.route_of(_shim(tmp_path_factory, DR), r)
    assert (got["regular"], got["marker"], got["redo"]) == DECODE_SITE[layout], (got["regular"], got["marker"], got["redo"], kernels)
    if got["redo"] != "none":
        assert got["redo_only"] == 1 and "k_decode_varint" in kernels      # dv_stream runs only on chunks the stream kernel hands back
    if layout in V.POINT_DECODER_LAYOUTS:
        assert got["nops"] == V.n_floatn(layout) and got["nf"] == 0 and got["tail"] == 1      # a hand-back: decode_varint_body<4, false> in k_decode_tail


_shims = {}


def _shim(factory, module):
    if module.__name__ not in _shims:
        _shims[module.__name__] = module.build_shim(factory.mktemp(module.__name__))
    return _shims[module.__name__]
