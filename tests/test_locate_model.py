"""No GPU: tests/locate_model.py (k_locate_sections restated in numpy) held to the oracle, and every row of tests/locate_cases.py
proved to take the branch its name says -- which is what keeps tests/test_gpu_locate.py from checking nothing."""
import numpy as np
import pytest

import cases
import locate_cases as LC
import locate_model as M
from cloudini_amd import synth

IDS = [c.name for c in LC.CASES]


def nw_of(case):
    return int(case.name[2:case.name.index("_")])


def frame(payload):
    return np.concatenate([np.frombuffer(np.uint32(len(payload)).tobytes(), np.uint8), np.asarray(payload, dtype=np.uint8)])


def oracle_regular_end(oracle, info, n_lanes, stream, n):
    """Where the oracle's own decode of the regular stream ends: the one prefix of the payload that a schema of the float lanes
    alone decodes to the same floats -- a byte less is an error (bytes behind the last point are not that decoder's business:
    the sections of the full schema must begin there, which the oracle's decode of the whole stream has shown)."""
    floats = info.copy(fields=info.fields[:n_lanes])
    want = oracle.decode_stage1(info, stream, n).reshape(n, info.point_step)[:, :4 * n_lanes]
    payload = stream[4:]
    ends = M.token_ends(payload)
    cut = int(ends[n * n_lanes - 1]) + 1
    got = oracle.decode_stage1(floats, frame(payload[:cut]), n).reshape(n, info.point_step)[:, :4 * n_lanes]
    assert np.array_equal(got, want)
    with pytest.raises(Exception):
        oracle.decode_stage1(floats, frame(payload[:cut - 1]), n)
    return cut


def test_the_trace_hook_stays_outside_the_boundary():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "cldn_hip_debug" not in open(os.path.join(root, "include", "cloudini_hip.h")).read()
    from cloudini_amd import native
    assert hasattr(native.lib(), "cldn_hip_debug_decode_trace")


def test_the_table_is_complete():
    assert len(set(IDS)) == len(IDS) == 52
    for nw in (4, 16):
        mine = [c for c in LC.CASES if nw_of(c) == nw]
        assert len(mine) == 26
        assert {c.branch for c in mine} == {"front", "dv_end", "drle_end"}
        assert {c.schema for c in mine} == set(LC.SCHEMAS)
        for c in mine:
            assert c.n <= 32768 and (nw == 4 or c.n >= 12000)


@pytest.mark.parametrize("case", LC.CASES, ids=IDS)
def test_every_case_takes_the_branch_its_name_says(oracle, case):
    nw = nw_of(case)
    info, cloud, stream, payload = case.build(oracle)
    _, lanes, ints = LC.schema(case.schema, case.n)
    n, n_ops, bpvs = case.n, len(lanes), [b for _, b in ints]
    oracle.decode_stage1(info, stream, n)                       # a valid stream
    loc = M.locate(payload, n, n_ops, bpvs, nw)
    # the plain token count is the oracle's: its decoder's regular stream ends there, and (streams the oracle wrote) the stream
    # of the float lanes alone has that many bytes
    assert loc.truth == oracle_regular_end(oracle, info, n_ops, stream, n)
    if not case.assemble:
        floats = info.copy(fields=info.fields[:n_ops])
        assert loc.truth == len(oracle.encode_stage1(floats, cloud)) - 4
    assert M.sections_decode_from(payload, loc.truth, n, bpvs)
    assert loc.branch == case.branch and loc.right == case.right, (loc, case.note)
    if loc.branch == "front":
        assert loc.reg_end_pre == loc.truth
    elif loc.right:
        assert loc.reg_end_pre == loc.truth                     # a guess the model calls right is the oracle's offset
    else:
        assert loc.reg_end_pre != loc.truth
    assert loc.mode_byte == (payload[loc.reg_end_pre] if loc.reg_end_pre < len(payload) else 0xFF)
    if case.size is not None:
        assert len(payload) == case.size
    if case.section is not None:
        assert len(payload) - loc.truth == case.section
    tile = LC.TILE[nw]
    # ---- what the name promises beyond the branch
    name = case.name[case.name.index("_") + 1:]
    behind = len(payload) - 1 - loc.truth                        # bytes behind the real mode byte
    if name.startswith("dv_") and case.right and case.branch == "dv_end":
        assert loc.dv_candidate == loc.truth and len(payload) >= tile + 16
    if name == "dv_size_tile_plus_15":
        assert len(payload) == tile + 15 and loc.dv_candidate is None
    if name == "dv_size_tile_plus_16":
        assert len(payload) == tile + 16
    for k in (1, 2, 3):
        if name == "dv_tile%d" % k:
            assert (k - 1) * tile <= behind < k * tile and len(payload) - (k - 1) * tile >= tile + 16
    if name == "dv_thread_first_byte":
        assert behind % 64 == 63
    if name == "dv_thread_last_byte":
        assert behind % 64 == 0
    if name == "dv_unit_first_byte":
        assert behind % 16 == 15 and behind % 64 != 63
    if name == "dv_unit_last_byte":
        assert behind % 16 == 0 and behind % 64 != 0
    if name == "dv_tile_lowest_byte":
        assert behind == tile - 1
    if name == "dv_standing_still":
        assert loc.truth == n * n_ops
    if name == "dv_in_front_of_the_tiles":
        reach = len(payload) - tile * ((len(payload) - 16) // tile)    # the lowest byte a tile covers
        assert loc.dv_candidate is None and loc.truth < reach and payload[loc.truth] == 0 and len(payload) >= tile + 16
    if name == "dv_refused_at_too_small":
        assert loc.dv_candidate is not None and payload[loc.dv_candidate] == 0 and loc.dv_candidate < n * n_ops
    if name == "dv_refused_no_mode_byte":
        assert loc.dv_candidate is not None and payload[loc.dv_candidate] != 0 and loc.dv_candidate >= n * n_ops
    if name == "dv_refused_not_closed":
        assert payload[-1] & 0x80 and payload[loc.truth] == 1 and int(payload[loc.truth + 1]) | int(payload[loc.truth + 2]) << 8 > 1024
    if name.startswith("dv_wrong"):
        at = loc.reg_end_pre
        assert payload[at] == 0 and n * n_ops <= at < loc.truth
        # (b): the bytes behind the false mode byte ARE a DeltaVarint section of n values, whoever decodes them
        assert M.sections_decode_from(payload, at, n, bpvs) == (name == "dv_wrong_garbage_column")
        zeros_behind = int((payload[at + 1:loc.truth] == 0).sum())
        assert (zeros_behind > 0) == (name == "dv_wrong_markers_behind")     # (b): the false mode byte is the LAST marker
        assert M.dv_w_completes(payload, at, n) == (name == "dv_wrong_garbage_column")
    if name.startswith("drle_"):
        assert len(payload) >= tile + 16                         # the DeltaVarint guess is tried whenever this one steps aside
    if name == "drle_ring":
        assert payload[loc.truth] == 3 and len(payload) - loc.truth <= LC.WINDOW[nw]
    if name == "drle_longer_than_window":
        assert payload[loc.truth] == 3 and len(payload) - loc.truth > LC.WINDOW[nw] and loc.drle_candidates == 0
    if name == "drle_false_alone":
        at = loc.reg_end_pre
        assert bytes(payload[at:at + 5]) == b"\x03\x0b\x00\x00\x00" and payload[loc.truth] == 2 and loc.drle_candidates == 1
        assert not M.sections_decode_from(payload, at, n, bpvs)
    if name == "drle_false_next_to_real":
        assert loc.drle_candidates == 2 and payload[loc.truth] == 3 and b"\x03\x0b\x00\x00\x00" in bytes(payload[:loc.truth])
    if name.startswith("front_part"):
        part = M.front_part_bytes(len(payload), nw)
        assert len(payload) % 16 != 0 and 0 < case.part_k < nw
        assert loc.truth == case.part_k * part + (1 if name.endswith("first_byte") else 0)
    if name == "front_two_fields":
        assert len(bpvs) == 2
    if name == "front_4ops_rle":
        assert n_ops == 4 and payload[loc.truth] == 2
    # ---- the trace behind the whole call, as the table states it
    oc = M.outcome(payload, n, n_ops, bpvs, loc)
    assert (oc.sec_cols, oc.sec_done, oc.dv_chunks) == (case.cols, case.sec_done, case.dv_chunks)
    assert oc.reg_end == loc.truth and oc.words[:4] == (1, 1, 0, 0)


@pytest.mark.parametrize("schema_name", sorted(LC.SCHEMAS))
def test_the_filler_cloud_is_located_from_the_front(oracle, schema_name):
    info, cloud, stream, payload = LC.filler(oracle, schema_name)
    _, lanes, ints = LC.schema(schema_name, 40)
    loc = M.locate(payload, 40, len(lanes), [b for _, b in ints], 4)
    assert loc.branch == "front" and loc.reg_end_pre == loc.truth == len(lanes) * 40


def test_early_returns_and_the_palette_branch(oracle):
    payload = np.ones(100, dtype=np.uint8)
    for bpvs in ([], [2] * 9, [8], [2, 8]):
        loc = M.locate(payload, 10, 3, bpvs, 4)
        assert (loc.branch, loc.reg_end_pre, loc.mode_byte) == ("none", M.NOT_FOUND, 0xFF)
    assert M.locate(payload, 10, 3, [2], 4, valid=False).branch == "none"
    # the two clouds of test_section_guess_with_a_false_hit_in_the_token_stream (tests/test_gpu_decode.py): a standing-still cloud
    # whose bytes 01 01 01 read as a header of 257 entries
    n = 20000
    fields = [("x", 0, cases.F.FLOAT32, 0.001), ("y", 4, cases.F.FLOAT32, 0.001), ("z", 8, cases.F.FLOAT32, 0.001),
              ("i", 12, cases.F.UINT16, None)]
    info = cases.make_info(fields, 16, n)
    rs = np.random.RandomState(5)
    for field in ("palette3", "growing"):
        vals = (rs.randint(0, 3, n) * 11).astype(np.uint16) if field == "palette3" else (np.arange(n) * 3 % 60000).astype(np.uint16)
        data = cases.pack(info, {"x": np.full(n, 1.5, np.float32), "y": np.full(n, -2.25, np.float32),
                                 "z": np.full(n, 0.75, np.float32), "i": vals}, n)
        payload = oracle.encode_stage1(info, data)[4:]
        for nw in (4, 16):
            loc = M.locate(payload, n, 3, [2], nw)
            kept = M.locate(payload, n, 3, [2], nw, keep_guess=1)
            if field == "palette3":     # the smaller, real hit wins: the kernel leaves the chunk to the point kernel's own guess
                assert (loc.branch, loc.right, loc.reg_end_pre, loc.mode_byte) == ("palette", True, M.NOT_FOUND, 0xFF)
                assert (kept.reg_end_pre, kept.mode_byte) == (loc.truth, 1)
                assert M.outcome(payload, n, 3, [2], loc).words == (1, 1, 0, 0, 1, 0, 0, 0)
            else:                       # 257 equal entries 01 01: the look-alike fails its checks, the run section is found instead
                assert M.pal_guess_from_end(payload, n, 2) is None
                assert (loc.branch, loc.right) == ("drle_end", True)
                assert M.outcome(payload, n, 3, [2], loc).words == (1, 1, 0, 0, 0, 0, 0, 0)


def test_palette_guess_rounds_and_checks():
    """pal_guess_from_end on hand-made payloads: each of its three checks refuses a look-alike and the next candidate is tried;
    four refusals end the search."""
    n, bpv = 64, 2

    def section(u, entries=None, indexes=None):
        bits = M.palette_bits(u)
        entries = list(range(100, 100 + u)) if entries is None else entries
        indexes = [k % u for k in range(n)] if indexes is None else indexes
        acc = sum(int(ix) << (bits * k) for k, ix in enumerate(indexes))
        body = b"".join(int(e).to_bytes(bpv, "little") for e in entries) + acc.to_bytes((bits * n + 7) // 8, "little")
        return np.frombuffer(bytes([1, u & 0xFF, u >> 8]) + body, dtype=np.uint8)

    front = np.full(400, 0x01, dtype=np.uint8)
    good = np.concatenate([front, section(5)])
    assert M.pal_guess_from_end(good, n, bpv) == 5
    unfinished = good.copy()
    unfinished[len(front) - 1] = 0x81                       # the token in front of the header is not over
    assert M.pal_guess_from_end(unfinished, n, bpv) is None
    assert M.pal_guess_from_end(np.concatenate([front, section(5, indexes=[7] + [0] * (n - 1))]), n, bpv) is None   # index >= U
    assert M.pal_guess_from_end(np.concatenate([front, section(5, entries=[9, 8, 9, 7, 6])]), n, bpv) is None       # entries repeat
    # look-alikes of 1, 2, 3 and 6 entries (5, 15, 25 and 39 bytes from the end) inside a real section of 9 entries (53 bytes):
    # each follows a byte that ends no token, is refused, and the next larger candidate is tried -- four times at the most
    for fakes, want in (((1,), 9), ((1, 2, 3), 9), ((1, 2, 3, 6), None)):
        p = np.concatenate([front, section(9, indexes=[0] * n)])
        for u in fakes:
            h = len(p) - M._palette_size(u, bpv, n)
            p[h:h + 3] = [1, u, 0]
            p[h - 1] |= 0x80
        got = M.pal_guess_from_end(p, n, bpv)
        assert got == want, (fakes, got)
