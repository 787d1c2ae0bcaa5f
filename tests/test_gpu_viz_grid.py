"""The constructed grid of the viz pre-filter (tests/viz_grid_cases.py) on the GPU: k_viz_insert, k_viz_count, k_viz_offsets and
k_viz_gather against the C oracle, byte for byte -- single-cloud calls, batch calls with a guard span, device-resident calls at
enumerated misalignments, forced cloud groups, and the fused filter + encode. tests/test_viz_grid_cases.py proves on the CPU
that every case reaches the branch it is built for, and pins the oracle to the compiled reference on every cloud used here."""
import numpy as np
import pytest

import cases
import viz_grid_cases as G
import viz_table_model as M
from cloudini_amd.schema import FieldType as F

FAMS = list(G.FAMILIES)
_want = {}


def _codec():
    from cloudini_amd import native, synth
    return native.Codec(native.Plan(synth.lidar_xyz(1)[0]))     # the codec only lends device, stream, workspace


def _expected(oracle, case):
    """The oracle's survivors per cloud, computed once per case and left unchanged."""
    if case.name not in _want:
        want = [oracle.viz_preprocess(c, case.step, case.off, case.res) for c in case.clouds]
        for w in want:
            w.setflags(write=False)
        _want[case.name] = want
    return _want[case.name]


def _check_batch(codec, case, want, tag):
    got, kept, tail = codec.viz_preprocess_batch_host(case.clouds, case.step, case.off, case.res, guard=64)
    assert [int(k) for k in kept] == [w.size // case.step for w in want], (case.name, tag)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size and np.array_equal(g, w), (case.name, tag, "cloud", k)
    assert np.all(tail == 0xA5), (case.name, tag, "behind the last survivor: the rest of the capacity and the guard")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
def test_single_cloud_calls(oracle, fam):
    codec = _codec()
    seen = set()
    for case in G.family(fam):
        for k, (c, w) in enumerate(zip(case.clouds, _expected(oracle, case))):
            if c.tobytes() in seen:                              # (the reversed batches, the one-point clouds)
                continue
            seen.add(c.tobytes())
            got = codec.viz_preprocess_host(c, case.step, case.off, case.res)
            assert got.size == w.size and np.array_equal(got, w), (case.name, "cloud", k, got.size // case.step, w.size // case.step)
    codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
def test_batch_calls(oracle, fam):
    codec = _codec()
    for case in G.family(fam):
        _check_batch(codec, case, _expected(oracle, case), "batch")
    codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.family("h"), ids=[c.name for c in G.family("h")])
def test_device_resident_at_every_misalignment(oracle, case):
    """Family h: input and output each 0, 4 and 1 bytes off a 256-byte aligned base (the alignment the model's branch names
    assume), 0xA5 in front of and behind the survivors."""
    import torch
    codec = _codec()
    dev = torch.device("cuda", 0)
    step = case.step
    data = np.concatenate(case.clouds)
    npts = np.array([c.size // step for c in case.clouds], dtype=np.uint64)
    flat = np.concatenate(_expected(oracle, case))
    front = 64
    for mi in G.MISALIGN:
        for mo in G.MISALIGN:
            d_in = torch.zeros(data.size + 16, dtype=torch.uint8, device=dev)
            d_out = torch.full((front + data.size + 16 + 256,), 0xA5, dtype=torch.uint8, device=dev)
            assert d_in.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0, "the caching allocator's base alignment"
            d_in[mi:mi + data.size] = torch.from_numpy(data).to(dev)
            torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
            kept = codec.viz_preprocess_batch_device(d_in.data_ptr() + mi, npts, step, case.off, case.res,
                                                     d_out.data_ptr() + front + mo, data.size)
            codec.synchronize()
            assert int(kept.sum()) * step == flat.size, (case.name, mi, mo)
            out = d_out.cpu().numpy()
            at = front + mo
            assert np.array_equal(out[at:at + flat.size], flat), (case.name, mi, mo)
            assert np.all(out[:at] == 0xA5) and np.all(out[at + flat.size:] == 0xA5), (case.name, mi, mo, "guard bytes")
    codec.close()


@pytest.mark.gpu
def test_forced_cloud_groups(oracle):
    """Family i with every non-empty cloud a group of its own, with at most two tables per group, and with the default: the
    tables of a group lie behind each other, so a chain that wraps ends right in front of the next cloud's first slots."""
    codec = _codec()
    for case in G.family("i"):
        want = _expected(oracle, case)
        two = 2 * max(M.capacity(c.size // case.step) for c in case.clouds)
        for slots, tag in ((1, "one cloud per group"), (two, "two tables per group"), (0, "default")):
            codec.viz_group_slots(slots)
            _check_batch(codec, case, want, tag)
    codec.close()


def _assert_same(got, want, tag):
    (gs, gc, gm, gk), (ws, wc, wm, wk) = got, want
    assert [int(k) for k in gk] == [int(k) for k in wk], (tag, "kept_points")
    assert len(gs) == len(ws)
    for k, (a, b) in enumerate(zip(gs, ws)):
        assert a.size == b.size and np.array_equal(a, b), (tag, "stream", k)
    assert np.array_equal(gc, wc), (tag, "chunk_sizes")
    assert np.array_equal(gm, wm), (tag, "modes")


def _fused_batch(fam):
    """One batch per family: the clouds of its cases that share the first case's (step, offset, resolution), up to 8192
    points, and the schema that gives the triple that resolution (the other bytes: UINT32 fields where four of them fit)."""
    first = G.family(fam)[0] if fam != "h" else [c for c in G.family("h") if c.step == 20][0]
    clouds, total = [], 0
    for case in G.family(fam):
        if (case.step, case.off, case.res) != (first.step, first.off, first.res):
            continue
        for c in case.clouds:
            if total + c.size // case.step <= 8192 and len(clouds) < 24:
                clouds.append(c)
                total += c.size // case.step
    step, off, res = first.step, first.off, first.res
    fields = [("x", off, F.FLOAT32, res), ("y", off + 4, F.FLOAT32, res), ("z", off + 8, F.FLOAT32, res)]
    fields += [(f"u{o}", o, F.UINT32, None) for o in list(range(0, off - 3, 4)) + list(range(off + 12, step - 3, 4))]
    return cases.make_info(fields, step, 0), clouds, off, res


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
def test_fused_filter_and_encode(oracle, fam):
    """encode_viz, contiguous and gather, against the plain encode of the oracle-filtered clouds (streams, chunk sizes,
    modes, kept counts): the comparison of tests/test_viz_batch.py."""
    from cloudini_amd import native
    info, clouds, off, res = _fused_batch(fam)
    assert clouds, fam
    step = info.point_step
    filtered = [oracle.viz_preprocess(c, step, off, res) for c in clouds]
    kept = np.array([f.size // step for f in filtered], dtype=np.uint64)
    plan = native.Plan(info)
    ref_codec, codec = native.Codec(plan), native.Codec(plan)
    want = ref_codec.encode_host(filtered) + (kept,)
    _assert_same(codec.encode_viz(clouds, off, res), want, (fam, "contiguous"))
    _assert_same(codec.encode_viz(clouds, off, res, gather=True), want, (fam, "gather"))
    codec.close()
    ref_codec.close()


@pytest.mark.gpu
def test_a_cloud_of_more_than_2_30_points_is_refused():
    """A table of 2^32 slots (more than 2^30 points) has a slot whose 32-bit index reads as "dropped", and from 2^31 points on
    the index is truncated. Refused behind the two older limits, before anything is allocated or read (null pointers)."""
    from cloudini_amd import native
    codec = _codec()
    text = "viz_preprocess: more than 2^30 points in one cloud"
    for counts in ([2 ** 30 + 1], [7, 2 ** 30 + 1, 7], [2 ** 31]):
        with pytest.raises(native.CloudiniHipError) as e:
            codec.viz_preprocess_batch_device(0, np.array(counts, dtype=np.uint64), 16, 0, 0.01, 0, 0)
        assert e.value.code == -3 and e.value.message == text, counts
    with pytest.raises(native.CloudiniHipError) as e:
        codec.viz_preprocess_device(0, 2 ** 30 + 1, 16, 0, 0.01, 0, 0)
    assert e.value.code == -3 and e.value.message == text
    with pytest.raises(native.CloudiniHipError) as e:           # the fused call shares the checks (the plan's step: 12)
        codec.encode_viz_device(0, np.array([2 ** 30 + 1], dtype=np.uint64), 0, 0.01, 0, 0)
    assert e.value.code == -3 and e.value.message == text
    # 2^30 points pass the limits: the call gets as far as its buffers, which are null here
    for call in (lambda: codec.viz_preprocess_batch_device(0, np.array([2 ** 30], dtype=np.uint64), 16, 0, 0.01, 0, 0),
                 lambda: codec.viz_preprocess_device(0, 2 ** 30, 16, 0, 0.01, 0, 0)):
        with pytest.raises(native.CloudiniHipError) as e:
            call()
        assert e.value.code != -3 and e.value.message == "viz_preprocess: NULL buffer"
    # the older limits answer first
    with pytest.raises(native.CloudiniHipError) as e:
        codec.viz_preprocess_batch_device(0, np.array([2 ** 31, 2 ** 31], dtype=np.uint64), 16, 0, 0.01, 0, 0)
    assert e.value.message == "viz_preprocess: more than 2^32 - 2 points in one batch"
    with pytest.raises(native.CloudiniHipError) as e:
        codec.viz_preprocess_batch_device(0, np.array([2 ** 30 + 1, 2 ** 32 - 1], dtype=np.uint64), 16, 0, 0.01, 0, 0)
    assert e.value.message == "viz_preprocess: more than 2^32 - 2 points"
    codec.close()
