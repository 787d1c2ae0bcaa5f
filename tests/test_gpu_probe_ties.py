"""GPU: the mode probe at near ties -- the three kernels that run probe_mode_t (cloudini_amd/csrc/stage1_sections.h) and the mode
sweep's own sizes and selection (mode_kernels.hip) on the grid of tests/probe_tie_cases.py. The probe returns only an argmin, so a
size that is off by one shows nowhere but on columns whose two smallest sizes lie within a byte of each other; the grid is such
columns, and tests/test_probe_tie_cases.py (CPU) proves that a one-byte error in any size changes the verdict on some of them.

One cloud per row, all rows of a field type in one call (blockIdx -> (cloud, field) over thousands of probe workgroups). Per
batch: file order twice on one codec (the second call runs under the first call's mode hints), and the reversed order with a
zero-point cloud inserted on a fresh codec. Every leg names its route through the shim of tests/test_encode_route.py and asserts
the route's `probe` field, so that a change of route cannot quietly drop a leg:
  a  probe == pieces  the probe workgroups of k_encode_fused (256 threads, 16 values each, AoS loads; 16- and 32-bit fields)
  b  probe == fast    k_probe_fast (1024 threads, 4 values each, column loads; every width)
  c  probe == wide    k_wide_probe (1024 threads, AoS loads; every width)
Asserted per call: the returned modes are the model's verdict and the oracle's probed modes, every stream is the oracle's bytes,
the codec's status is OK. The route is computed from the facts this file passes to the call (tests/test_encode_route.abi_facts),
not read back from the codec; tools/encode_route_trace.py holds the two together on kernel traces."""
import numpy as np
import pytest

import cases
import mode_cases as MC
import mode_model as M
import probe_tie_cases as P
import test_encode_route as TR

pytestmark = pytest.mark.gpu

F = cases.F
XYZ = [("x", 0, F.FLOAT32, 0.001), ("y", 4, F.FLOAT32, 0.001), ("z", 8, F.FLOAT32, 0.001)]
_NP = P.NP
_xyz = {}
_expected = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return TR.build_shim(tmp_path_factory.mktemp("probe_tie_route"))


def _rows(ftype, *families):
    return [r for r in P.rows(*families) if r[2] == ftype]


def _xyz_cols(n):
    if "pts" not in _xyz:
        from cloudini_amd import synth
        _xyz["pts"] = synth.lidar_xyz(P.CHUNK + 300, seed=7)[1].view(np.float32).reshape(-1, 3)
    p = _xyz["pts"][:n]
    return {"x": p[:, 0], "y": p[:, 1], "z": p[:, 2]}


class Layout:
    """A schema and how a cloud is packed from one column per integer field. `ints`: (name, offset, type) of the adaptive fields."""

    def __init__(self, name, fields, step, ops):
        self.name, self.fields, self.step, self.ops = name, fields, step, ops
        self.ints = [f for f in fields if f[2] in _NP]
        self.adaptive = [(np.dtype(_NP[f[2]]).itemsize, f[1]) for f in self.ints]
        self.info = cases.make_info(fields, step, 1)

    def cloud(self, columns):
        """columns: one array per adaptive field, equal lengths."""
        n = len(columns[0])
        cols = dict(_xyz_cols(n)) if self.fields[0][0] == "x" else {}
        for f in self.fields:
            if f[2] == F.UINT8:
                cols[f[0]] = (np.arange(n) % 251).astype(np.uint8)
        for f, c in zip(self.ints, columns):
            cols[f[0]] = c
        return cases.pack(cases.make_info(self.fields, self.step, n), cols, n)


def xyz_one(ftype):
    w = P.WIDTH_OF[ftype]
    step = 16 if w < 8 else 24
    return Layout(f"xyz_{ftype.name}", XYZ + [("v", 12 if w < 8 else 16, ftype, None)], step, TR.xyz())


def xyz_u16_u32():
    return Layout("xyz_u16_u32", XYZ + [("a", 12, F.UINT16, None), ("b", 14, F.UINT32, None)], 18, TR.xyz())


def int_only(ftype, odd):
    w = P.WIDTH_OF[ftype]
    if not odd:
        return Layout(f"{ftype.name}_alone", [("value", 0, ftype, None)], w, [])
    return Layout(f"{ftype.name}_odd", [("p", 0, F.UINT8, None), ("value", 1, ftype, None)], 1 + w + 2, [(TR.COPY, 1, 0)])


def wide_layout(w):
    """XYZ and 65 integer fields of one width, unsigned and signed in turns: more adaptive fields than the ordinary plan holds."""
    fields = XYZ + [(f"f{k}", 12 + w * k, P.TYPES_OF[w][k % 2], None) for k in range(65)]
    return Layout(f"wide_65_w{w}", fields, 12 + 65 * w, [])


def _expect(oracle, layout, key, cloud):
    """(the oracle's stream, its probed modes, the model's verdicts) of one cloud, once per (layout, cloud)."""
    k = (layout.name, key)
    if k not in _expected:
        n = cloud.size // layout.step
        stream, probed = oracle.encode_stage1(layout.info, cloud, return_modes=True)
        model = M.sweep(layout.info, cloud, [n])["probe_mode"][0]
        assert probed.tolist() == model.tolist(), (layout.name, key)
        _expected[k] = (stream, probed)
    return _expected[k]


def _route(shim, layout, n_clouds, host, hints=None, **call):
    adaptive = [] if call.get("wide") else layout.adaptive          # (a wide plan's fields are not in the launch-argument plan)
    r = TR.row(layout.name, None, layout.step, layout.ops, adaptive, n_chunks=n_clouds, n_clouds=n_clouds,
               **({"hints": hints} if hints else {}), **call)
    return TR.route_of(shim, r, host_input=host)[1]


def _hints(modes):
    """What a call leaves as mode hints: per field the set of modes its clouds committed."""
    return [int(np.bitwise_or.reduce(1 << modes[:, a].astype(np.int64))) for a in range(modes.shape[1])]


def _check(what, keys, got_streams, got_modes, want):
    bad = [(k, g.tolist(), w[1].tolist()) for k, g, w in zip(keys, got_modes, want) if g.tolist() != w[1].tolist()]
    assert not bad and len(got_modes) == len(want), f"{what}: {len(bad)} clouds commit another mode; (row, got, want): {bad[:12]}"
    bad = [k for k, g, w in zip(keys, got_streams, want) if g.tobytes() != w[0].tobytes()]
    assert not bad and len(got_streams) == len(want), f"{what}: {len(bad)} streams are not the oracle's bytes: {bad[:12]}"


def _codec(layout, pipeline=0):
    from cloudini_amd import native
    codec = native.Codec(native.Plan(layout.info))
    if pipeline:
        assert codec.pipeline(pipeline) == pipeline
    return codec


def _run_host(oracle, shim, layout, batch, probe, pipeline=0, wide=None):
    """batch: [(key, cloud bytes)]. File order twice on one codec, reversed with a zero-point cloud on another."""
    na = len(layout.ints)
    zero = ("zero points", np.zeros(0, np.uint8))
    want = [_expect(oracle, layout, k, c) for k, c in batch]
    empty = (np.zeros(0, np.uint8), np.zeros(na, np.uint8))
    wide = wide or {}
    codec = _codec(layout, pipeline)
    hints = None
    for call in range(2):
        assert _route(shim, layout, len(batch), True, hints, pipeline=pipeline, **wide)["probe"] == probe, (layout.name, call)
        streams, _cs, modes = codec.encode_host([c for _k, c in batch])
        codec.status()
        _check((layout.name, "file order", call), [k for k, _c in batch], streams, modes, want)
        hints = None if wide else _hints(modes)
    codec.close()
    codec = _codec(layout, pipeline)
    rev = batch[::-1]
    rev = rev[:len(rev) // 2] + [zero] + rev[len(rev) // 2:]
    want_rev = want[::-1]
    want_rev = want_rev[:len(batch) // 2] + [empty] + want_rev[len(batch) // 2:]
    assert _route(shim, layout, len(batch), True, None, pipeline=pipeline, **wide)["probe"] == probe
    streams, _cs, modes = codec.encode_host([c for _k, c in rev])
    codec.status()
    _check((layout.name, "reversed"), [k for k, _c in rev], streams, modes, want_rev)
    codec.close()


def _run_device_modes_at_an_odd_address(oracle, shim, layout, batch, probe):
    """Device-resident points and output: the probe workgroups store the caller's modes array themselves."""
    import torch
    dev = torch.device("cuda", 0)
    na = len(layout.ints)
    want = [_expect(oracle, layout, k, c) for k, c in batch]
    sizes = [c.size // layout.step for _k, c in batch]
    got = _route(shim, layout, len(batch), False)
    assert got["probe"] == probe and got["writes_caller_modes"] == 1, layout.name
    codec = _codec(layout)
    flat = torch.from_numpy(np.concatenate([c for _k, c in batch])).to(dev)
    assert flat.data_ptr() % 4 == 0
    cap = sum(codec.plan.stage1_bound(n) for n in sizes)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(batch) + 1, dtype=torch.int64, device=dev)
    d_modes = torch.full((256 + len(batch) * na + 256,), 0xEE, dtype=torch.uint8, device=dev)
    at = (-d_modes.data_ptr()) % 256 + 1
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.encode_device(flat.data_ptr(), sizes, d_out.data_ptr(), cap, d_off.data_ptr(), 0, d_modes.data_ptr() + at)
    codec.status()
    torch.cuda.synchronize()
    o, h, m = d_off.cpu().numpy(), d_out.cpu().numpy(), d_modes.cpu().numpy()
    assert (m[:at] == 0xEE).all() and (m[at + len(batch) * na:] == 0xEE).all(), "the modes were written outside their array"
    _check((layout.name, "device"), [k for k, _c in batch], [h[int(o[k]):int(o[k + 1])] for k in range(len(batch))], m[at:at + len(batch) * na].reshape(-1, na), want)
    codec.close()


def _one_field_batch(layout, ftype, *families):
    return [(r[0], layout.cloud([r[3]])) for r in _rows(ftype, *families)]


# ---- leg a: the probe workgroups of the piece kernel ---------------------------------------------------------------------------

@pytest.mark.parametrize("ftype", [F.UINT16, F.INT16, F.UINT32, F.INT32], ids=lambda t: t.name)
def test_leg_a_pieces(oracle, shim, ftype):
    layout = xyz_one(ftype)
    batch = _one_field_batch(layout, ftype, "pair", "term", "tiny")
    assert len(batch) > 800
    _run_host(oracle, shim, layout, batch, "pieces")
    _run_device_modes_at_an_odd_address(oracle, shim, layout, batch, "pieces")


def _padded(values, n):
    """The row's window with its last value repeated up to n values: the probe sees the row."""
    assert values.size >= P.PROBE or values.size == n
    return np.concatenate([values, np.full(n - values.size, values[-1], values.dtype)])


def _two_field_batch(layout):
    """A 16-bit and a 32-bit row per cloud, different ones: rows of equal length side by side, and rows that fill the window
    (full, beyond) padded behind it to the longer of the two."""
    batch = []
    for fams, fits in ((("term",), lambda r: r[3].size == P.TERM_N), (("pair", "term"), lambda r: r[3].size >= P.PROBE)):
        a = [r for r in _rows(F.UINT16, *fams) if fits(r)]
        b = [r for r in _rows(F.UINT32, *fams) if fits(r)]
        assert len(a) >= 9 and len(b) >= 9
        for k in range(max(len(a), len(b))):
            ra, rb = a[k % len(a)], b[(k + 1) % len(b)]
            n = max(ra[3].size, rb[3].size)
            batch.append((ra[0] + "+" + rb[0], layout.cloud([_padded(ra[3], n), _padded(rb[3], n)])))
    return batch


def test_leg_a_pieces_two_probe_workgroups_per_cloud(oracle, shim):
    layout = xyz_u16_u32()
    batch = _two_field_batch(layout)
    got = _route(shim, layout, len(batch), True)
    assert got["n_probe"] == 2 * len(batch) and got["pieces_lds"] == TR.LDS_PROBE32
    _run_host(oracle, shim, layout, batch, "pieces")
    _run_device_modes_at_an_odd_address(oracle, shim, layout, batch, "pieces")


# ---- leg b: k_probe_fast ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ftype", MC.TYPES, ids=lambda t: t.name)
def test_leg_b_fast_behind_xyz(oracle, shim, ftype):
    """The schemas of leg a under pipeline 1 (the generic kernel: the probe is a kernel of its own), and a 64-bit field behind XYZ."""
    layout = xyz_one(ftype)
    _run_host(oracle, shim, layout, _one_field_batch(layout, ftype, "pair", "term"), "fast", pipeline=1)


def test_leg_b_fast_two_fields(oracle, shim):
    layout = xyz_u16_u32()
    _run_host(oracle, shim, layout, _two_field_batch(layout), "fast", pipeline=1)


@pytest.mark.parametrize("odd", [False, True], ids=["offset_0", "offset_1_of_an_odd_step"])
@pytest.mark.parametrize("ftype", MC.TYPES, ids=lambda t: t.name)
def test_leg_b_fast_integer_only(oracle, shim, ftype, odd):
    layout = int_only(ftype, odd)
    families = ("pair", "term") if odd else ("pair", "term", "tiny")
    _run_host(oracle, shim, layout, _one_field_batch(layout, ftype, *families), "fast", pipeline=1)


# ---- leg c: k_wide_probe ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", P.WIDTHS)
def test_leg_c_wide(oracle, shim, w):
    layout = wide_layout(w)
    from cloudini_amd import native
    assert native.Plan(layout.info).adaptive_fields == 65
    batch = []
    for k, r in enumerate(P.rows("pair", "term")):
        if P.WIDTH_OF[r[2]] != w:
            continue
        at = 2 * (k % 32) + (r[2] in P.SIGNED)                      # a field of the row's own type, another one from row to row
        n = r[3].size
        cols = [((np.arange(n) // (3 + j)) % 11).astype(_NP[f[2]]) for j, f in enumerate(layout.ints)]
        cols[at] = r[3]
        batch.append((r[0], layout.cloud(cols)))
    assert len(batch) > 100
    wide = dict(wide=1, wide_adaptive=65, max_regular_bytes=15)
    _run_host(oracle, shim, layout, batch, "wide", wide=wide)


# ---- the sweep's own sizes and selection ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ftype", MC.TYPES, ids=lambda t: t.name)
def test_sweep_sizes_probe_mode_and_best_mode(ftype):
    from cloudini_amd import native
    rows = _rows(ftype, "pair", "term", "sums")
    layout = int_only(ftype, False)
    clouds = [layout.cloud([r[3]]) for r in rows]
    sizes = [r[3].size for r in rows]
    want = M.sweep(layout.info, np.concatenate(clouds), sizes)
    for k, r in enumerate(rows):                                    # the model's cells are the rows' own figures
        assert want["bytes"][k, 0].tolist() == P.whole_sizes(r[3]) and want["probe_mode"][k, 0] == M.select(P.window_sizes(r[3]))
        assert want["best_mode"][k, 0] == M.select(P.whole_sizes(r[3]))
    codec = native.Codec(native.Plan(layout.info))
    got = codec.sweep_modes_host(clouds)
    for name in ("bytes", "probe_mode", "best_mode"):
        bad = [(rows[k][0], got[name][k, 0].tolist(), want[name][k, 0].tolist()) for k in range(len(rows))
               if got[name][k, 0].tolist() != want[name][k, 0].tolist()]
        assert not bad, f"{name}: {len(bad)} cells differ; (row, got, want): {bad[:12]}"
    codec.close()
