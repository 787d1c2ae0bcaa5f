"""The rule set of the device ZSTD decoder (tests/zstd_lit_rules.py) against the system libzstd, one-sided both ways:
  rules say OK      => ZSTD_decompress with room for exactly `capacity` bytes returns the same bytes
  rules say CORRUPT => ZSTD_decompress returns an error
  HOST claims nothing.
Inputs: tests/zstd_decode_cases.py (a grid frames, b libzstd-made frames, c hand-built frames, d damage). No GPU."""
import os

import zstd_decode_cases as K
import zstd_lit_rules as R


def pin(name, frame, capacity):
    verdict, payload = R.decode(frame, capacity)
    if verdict == R.OK:
        assert K.libzstd_decompress(frame, capacity) == payload, name
    elif verdict == R.CORRUPT:
        assert K.libzstd_decompress(frame, capacity) is None, name
    return verdict, payload


def test_grid_frames_are_ok():
    frames = K.grid_frames()
    assert len({n.split("/")[0] for n, *_ in frames}) == 39
    for name, frame, cap, payload in frames:
        assert pin(name, frame, cap) == (R.OK, payload), name
        assert R.decode(frame, cap - 1)[0] == R.CORRUPT or cap == 0


def kinds_of(frame, cap):
    _v, blocks, _t = R.walk(frame, cap)
    return blocks


def test_libzstd_frames():
    verdicts = {}
    treeless_ok = []
    for name, frame, cap, payload in K.libzstd_frames():
        v, out = pin(name, frame, cap)
        verdicts[name] = v
        if v == R.OK:
            assert out == payload, name
            if any(b["kind"] == R.HUF and b["desc"] == 0 for b in kinds_of(frame, cap)):
                treeless_ok.append(name)
    print({v: sum(1 for x in verdicts.values() if x == v) for v in (R.OK, R.HOST, R.CORRUPT)}, "treeless in OK frames:", treeless_ok)
    assert R.CORRUPT not in verdicts.values()
    assert verdicts["geometric/level1/300000"] == R.OK
    assert verdicts["zipf/level1/300000"] == R.HOST and verdicts["geometric/checksum/1023"] == R.HOST
    assert any(v == R.HOST and _stops_at_sequences(f, c) for (n, f, c, _p), v in zip(K.libzstd_frames(), verdicts.values()))
    for n in (0, 1, 63, 64, 255, 256, 1023, 131071, 131072, 131073):
        assert verdicts[f"random/level1/{n}"] == R.OK and verdicts[f"geometric/level1/{n}"] == R.OK, n
    # (a constant run: this libzstd codes it as one match, not as an RLE block -- HOST from 63 bytes on; RLE blocks are the
    # grid's and the hand-built frames')
    assert verdicts["constant/level1/1"] == R.OK and verdicts["constant/level1/1023"] == R.HOST
    # an OK frame of libzstd's own with a treeless block; where this libzstd writes none in a literal-only frame, the
    # hand-built ones of test_hand_built_frames carry that form
    assert treeless_ok or any(n.startswith("treeless/") for n, *_ in K.hand_frames())
    if not treeless_ok:
        print("libzstd wrote no treeless block in a literal-only frame here: hand_frames' treeless/* carry that form")


def _stops_at_sequences(frame, cap):
    note = {}
    return R.walk(frame, cap, note=note)[0] == R.HOST and note.get("why") == "sequences"


def test_hand_built_frames():
    seen = {}
    for name, frame, cap, payload in K.hand_frames():
        v, out = pin(name, frame, cap)
        seen[name] = v
        if payload is not None:
            assert (v, out) == (R.OK, payload), name
        else:
            assert v == (R.HOST if name.startswith("host/") else R.CORRUPT), (name, v)
    assert {"treeless/11", "treeless/10", "treeless/01", "treeless/first", "direct/5", "streams/one_255", "streams/four_256"} <= set(seen)
    assert all(f"header/{k}" in seen for k in ("single/1", "single/2", "single/4", "single/8", "window/0", "window/2", "window/4", "window/8"))


def test_damage():
    seed = int.from_bytes(os.urandom(4), "little") | 1
    cases = K.damaged(seed)
    counts = {R.OK: 0, R.HOST: 0, R.CORRUPT: 0}
    for name, frame, cap in cases:
        v, _ = pin(f"seed {seed} {name}", frame, cap)
        counts[v] += 1
    share = counts[R.HOST] / len(cases)
    print(f"damage: {len(cases)} frames (random seed {seed}), {counts}, HOST share {share:.3f}")
    assert share < 0.5 and counts[R.CORRUPT] > len(cases) // 4
