"""The rule set of the device ZSTD decoder with the sequences switch on (tests/zstd_seq_rules.py) against the system libzstd,
one-sided both ways:
  rules say OK      => ZSTD_decompress with room for exactly `capacity` bytes returns the same bytes
  rules say CORRUPT => ZSTD_decompress returns an error
  HOST claims nothing -- but it may not be a hiding place: of the libzstd-made frames every one libzstd accepts is OK (except
  with the checksum flag), of the constructed grid every one except those built for a named HOST rule.
It is a superset of tests/zstd_lit_rules.py: what that module calls OK or CORRUPT keeps verdict and bytes.
Inputs: tests/zstd_seq_cases.py and every set of tests/zstd_decode_cases.py. No GPU."""
import os

import zstd_decode_cases as K
import zstd_lit_rules as R
import zstd_seq_cases as Q
import zstd_seq_rules as S


def pin(name, frame, capacity):
    verdict, payload, trace = S.decode_trace(frame, capacity)
    if verdict == S.OK:
        assert K.libzstd_decompress(frame, capacity) == payload, name
    elif verdict == S.CORRUPT:
        assert K.libzstd_decompress(frame, capacity) is None, name
    return verdict, payload, trace


def test_constructed_grid():
    names = set()
    traces = {}
    for name, frame, cap, payload in Q.grid_frames():
        v, out, traces[name] = pin(name, frame, cap)
        names.add(name)
        if payload is not None:
            assert (v, out) == (S.OK, payload), name
        elif name in Q.HOST_BY_RULE:
            assert v == S.HOST, name
        else:
            assert v == S.CORRUPT, (name, v)
        if v == S.HOST:
            assert name in Q.HOST_BY_RULE, name
    # what the grid is there for, read from the model's trace (never its bytes)
    for ofv in (1, 2, 3):
        for ll0 in (True, False):
            assert (ofv, ll0) in traces[f"rep/{ofv}/ll{0 if ll0 else 2}"]["rep"]
    assert len(traces["rep/three_in_a_row"]["rep"]) >= 3
    assert traces["two_blocks/history"]["cross_block"] and traces["literals/treeless"]["cross_block"]
    assert [b["modes"] for b in traces["two_blocks/repeat_modes"]["blocks"]] == [(1, 1, 1), (3, 3, 3)]
    modes = {b["modes"] for n in ("two_blocks/repeat_modes", "two_blocks/repeat_some") for b in traces[n]["blocks"]}
    assert all(any(m[t] == S.REPEAT for m in modes) for t in range(3))
    # Repeat of a Predefined and of an FSE_Compressed table (libzstd wrote no Repeat here: hand-built, single-sequence blocks)
    assert [b["modes"] for b in traces["repeat_of/predefined"]["blocks"]] == [(0, 0, 0), (3, 3, 3)]
    assert [b["modes"] for b in traces["repeat_of/fse"]["blocks"]] == [(2, 2, 2), (3, 3, 3)]
    # state updates under Predefined and FSE tables: three sequences in a block (the order LL, ML, OF shows in chain/predefined)
    assert [(b["modes"], b["nb"]) for b in traces["chain/predefined"]["blocks"]] == [((0, 0, 0), 3)]
    assert [(b["modes"], b["nb"]) for b in traces["chain/fse"]["blocks"]] == [((2, 2, 2), 3)]
    assert traces["match/ml70000/off1"]["overlap"] and traces["match/ml3/off65/r10"]["max_offset"] == 65
    assert {traces[n]["blocks"][0]["form"] for n in ("count/one_in_two_bytes", "count/128", "count/three_bytes")} == {2, 3}
    assert traces["count/three_bytes"]["blocks"][0]["form"] == 3
    R = Q.ring()
    for n, reach in (("inside", R), ("outside_by_one", R + 1), ("straddling", R + 32), ("outside", R + 64)):
        for ml in (60, 200):
            t = traces[f"ring/{n}/ml{ml}"]
            assert t["max_offset"] == max(reach, R + 1900) and t["cross_block"] and sum(b["nb"] for b in t["blocks"]) == 3, (n, ml)
    assert traces["ring/periodic_outside"]["max_offset"] == R + 5 and traces["ring/periodic_outside"]["overlap"]
    assert traces["ring/second_block"]["max_offset"] == 180000
    assert {f"align/ml17/off3/r{r}" for r in range(16)} <= names


def _check_libzstd(frames):
    modes = [set(), set(), set()]
    forms = set()
    far = 0
    for name, frame, cap, payload in frames:
        v, out, trace = pin(name, frame, cap)
        if name in Q.LIBZSTD_HOST:                                        # the named exceptions: HOST by the record limit
            sums = S.walk(frame, cap, all_blocks=None, read_trees=False)[2]
            assert v == S.HOST and sums["n_all"] > S.record_limit(len(frame), cap, True), name
            continue
        assert (v, out) == (S.OK, payload), name                      # HOST is no hiding place
        for b in trace["blocks"]:
            forms.add(b["form"])
            for t in range(3):
                modes[t].add(b["modes"][t])
        far = max(far, trace["max_offset"])
    return modes, forms, far


def test_libzstd_frames(oracle):
    modes, forms, far = _check_libzstd(Q.libzstd_frames() + Q.lidar_frames(oracle))
    print("modes libzstd wrote for LL / OF / ML:", modes, "count forms:", forms, "largest offset:", far)
    # what this libzstd does not write over these sources is the constructed grid's: say which
    grid = {}
    for name, frame, cap, _p in Q.grid_frames():
        grid[name] = S.decode_trace(frame, cap)[2]
    for t in range(3):
        have = set(modes[t])
        for name in ("two_blocks/repeat_modes", "two_blocks/repeat_some", "ll/0"):
            have |= {b["modes"][t] for b in grid[name]["blocks"]}
        missing = {S.PREDEFINED, S.MODE_RLE, S.FSE, S.REPEAT} - set(modes[t])
        if missing:
            print(f"table {t}: libzstd wrote no mode {sorted(missing)} here; the constructed grid carries RLE and Repeat")
        assert have == {S.PREDEFINED, S.MODE_RLE, S.FSE, S.REPEAT}, (t, have)
        assert {S.PREDEFINED, S.FSE} <= modes[t], (t, modes[t])           # (no hand-built frame has these two)
    assert {1, 2} <= forms                                                # (the 3-byte form: count/three_bytes of the grid)
    assert far > 65536


def test_frames_of_the_literal_decoder_keep_their_verdicts():
    """the superset property, over every input set of zstd_decode_cases"""
    seed = int.from_bytes(os.urandom(4), "little") | 1
    cases = [(n, f, c) for n, f, c, _p in K.grid_frames() + K.libzstd_frames() + K.hand_frames()] + K.damaged(seed)
    judged = 0
    for name, frame, cap in cases:
        old = R.decode(frame, cap)
        new = pin(f"seed {seed} {name}", frame, cap)[:2]
        if old[0] != R.HOST:
            assert new == old, (seed, name)
        else:
            judged += new[0] != S.HOST
    print(f"{len(cases)} frames (random seed {seed}); {judged} that were HOST are judged now")
    assert judged > 10
    v = {n: S.decode(f, c)[0] for n, f, c, _p in K.libzstd_frames()}
    assert v["zipf/level1/300000"] == S.OK and v["constant/level1/1023"] == S.OK and v["geometric/checksum/1023"] == S.HOST


def test_damage():
    cases = [c for i in range(len(Q.damage_bases())) for c in Q.damaged_base(i)] + Q.random_damage()
    counts = {S.OK: 0, S.HOST: 0, S.CORRUPT: 0}
    for name, frame, cap in cases:
        counts[pin(name, frame, cap)[0]] += 1
    share = counts[S.HOST] / len(cases)
    print(f"damage: {len(cases)} frames, {counts}, HOST share {share:.3f}")
    assert len(Q.damage_bases()) <= 8 and share < 0.5 and counts[S.CORRUPT] > len(cases) // 4
