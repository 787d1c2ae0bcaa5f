"""GPU: which branch of k_locate_sections (stage1_decode_fast.h) located every chunk, and how a wrong guess was recovered from.
Byte parity with the oracle cannot see either -- a dead shortcut and a working safety net give the same bytes -- so every case of
tests/locate_cases.py is decoded by a fresh codec (no launch hints) and the trace of the call (cldn_hip_debug_decode_trace: the
status words 8..15 and the per-chunk arrays of the workspace) is held against tests/locate_model.py, chunk by chunk. The CPU test
tests/test_locate_model.py proves that every case takes the branch its name says; nothing is skipped or filtered here.

NW = 16 (k_locate_sections<16>, at most 64 chunks in the call): the case's cloud alone. NW = 4: the cloud and 64 small clouds."""
import numpy as np
import pytest

import locate_cases as LC
import locate_model as M

pytestmark = pytest.mark.gpu

RUNS = [(c, split) for c in LC.CASES for split in (c.split if c.name.startswith("nw16_") else (0,))]
FILL = 0x5A


@pytest.fixture(scope="module")
def fillers(oracle):
    """Per schema: the filler cloud's stream, its decode and its trace (locate_model)."""
    res = {}
    for name in LC.SCHEMAS:
        info, _cloud, stream, payload = LC.filler(oracle, name)
        _, lanes, ints = LC.schema(name, 40)
        bpvs = [b for _, b in ints]
        loc = M.locate(payload, 40, len(lanes), bpvs, 4)
        res[name] = (stream, oracle.decode_stage1(info, stream, 40, fill=FILL), loc, M.outcome(payload, 40, len(lanes), bpvs, loc))
    return res


@pytest.mark.parametrize("case,split", RUNS, ids=["%s-split%d" % (c.name, s) for c, s in RUNS])
def test_trace_of_a_decode_call_equals_the_model(oracle, fillers, case, split):
    from cloudini_amd import native
    nw = 16 if case.name.startswith("nw16_") else 4
    info, _cloud, stream, payload = case.build(oracle)
    _, lanes, ints = LC.schema(case.schema, case.n)
    n, n_ops, bpvs = case.n, len(lanes), [b for _, b in ints]
    loc = M.locate(payload, n, n_ops, bpvs, nw)
    assert loc.branch == case.branch and loc.right == case.right      # (tests/test_locate_model.py has the details)
    want = [(oracle.decode_stage1(info, stream, n, fill=FILL), loc, M.outcome(payload, n, n_ops, bpvs, loc))]
    streams, npts = [stream], [n]
    if nw == 4:
        f_stream, f_want, f_loc, f_out = fillers[case.schema]
        streams += [f_stream] * LC.FILLERS
        npts += [40] * LC.FILLERS
        want += [(f_want, f_loc, f_out)] * LC.FILLERS
    codec = native.Codec(native.Plan(info))
    if split:
        assert codec.decode_split(split) == 0
    for call in range(2):      # the second call: the first one's hints have landed, a column left from it would show
        out = np.full(sum(npts) * info.point_step, FILL, dtype=np.uint8)
        got = codec.decode_host(streams, npts, out=out)
        for k, (w, _l, _o) in enumerate(want):
            assert np.array_equal(got[k], w), (call, k, int(np.nonzero(got[k] != w)[0][0]))
        if call:
            break
        tr = codec.decode_trace()
        assert tr["n_chunks"] == len(want)
        for k, (_w, l, o) in enumerate(want):
            seen = (int(tr["reg_end_pre"][k]), int(tr["slices_done"][k]) >> 24, int(tr["sec_cols"][k]), int(tr["reg_end"][k]),
                    int(tr["sec_done"][k]))
            assert seen == (l.reg_end_pre, l.mode_byte, o.sec_cols, o.reg_end, o.sec_done), (k, l.branch, seen)
        words = tuple(sum(o.words[i] for _w, _l, o in want) for i in range(8))
        assert tr["words"] == words, (tr["words"], words)
        assert tr["words"][7] == sum(l.branch == "dv_end" for _w, l, _o in want)
    codec.close()
