"""Crafted integer columns for the adaptive mode sweep, shared by tests/test_mode_model.py (model against oracle and reference)
and tests/test_gpu_modes.py (device against model). Each case names the condition it was built for as a check on the MODEL:
check(v) is False when the column does not have the property, so a case can never pass for the wrong reason.

The shapes are the smallest that reach the edges of mode_kernels.hip: waves of 64 values, stages of 1024 values (fewer for
wide points), chunks of 32768, the LDS table of one hash partition (10240 keys of 32 bits, 5120 of 64 bits), the growth of the
partition count (1, the run-count rule, doubling up to 64) and the direct count behind it."""
from __future__ import annotations

import numpy as np

import cases
import mode_model as M

F = cases.F
CHUNK = M.CHUNK
TYPES = [F.UINT16, F.INT16, F.UINT32, F.INT32, F.UINT64, F.INT64]
_NP = {F.UINT16: np.uint16, F.INT16: np.int16, F.UINT32: np.uint32, F.INT32: np.int32, F.UINT64: np.uint64, F.INT64: np.int64}
PAL_CAP = {4: 10240, 8: 5120}  # keys one pass of the kernel's 64 KiB table may hold, by key width
PAL_MAX_PARTS = 64              # more partitions are not tried: the kernel counts first occurrences directly
DIRECT = 0                      # partitions_needed: the hash never separated the keys
_M64 = (1 << 64) - 1


def mix(v):
    """mode_mix of mode_kernels.hip on the raw (zero-extended) bits: partition = low bits, table slot = bits 40.."""
    v = v.astype(np.uint64)
    v = v ^ (v >> np.uint64(30))
    v = v * np.uint64(0xbf58476d1ce4e5b9)
    v = v ^ (v >> np.uint64(27))
    v = v * np.uint64(0x94d049bb133111eb)
    return v ^ (v >> np.uint64(31))


def unmix(m):
    """The inverse of mix (it is a bijection of 64-bit words): the key whose mix is m."""
    m = np.asarray(m, dtype=np.uint64)
    m = m ^ (m >> np.uint64(31)) ^ (m >> np.uint64(62))
    m = m * np.uint64(pow(0x94d049bb133111eb, -1, 1 << 64))
    m = m ^ (m >> np.uint64(27)) ^ (m >> np.uint64(54))
    m = m * np.uint64(pow(0xbf58476d1ce4e5b9, -1, 1 << 64))
    return m ^ (m >> np.uint64(30)) ^ (m >> np.uint64(60))


def run_count_rule(raw, width):
    """The partition count of the kernel's second attempt: from the Rle run count alone."""
    cap = PAL_CAP[width]
    runs = 1 + int((raw[1:] != raw[:-1]).sum())
    parts = 2
    while runs // parts > cap - cap // 8:
        parts *= 2
    return parts


def partitions_needed(raw, width):
    """How many hash partitions the kernel ends with for one section of raw values: 1 if the distinct non-zero values fit one
    pass, else the power of two >= 2 that the Rle run count asks for with an eighth of headroom, doubled while a partition
    overflows; DIRECT when PAL_MAX_PARTS partitions still overflow."""
    cap = PAL_CAP[width]
    keys = np.unique(raw.astype(np.uint64))
    keys = keys[keys != 0]
    fits = lambda parts: np.bincount((mix(keys) & np.uint64(parts - 1)).astype(np.int64), minlength=parts).max() <= cap
    if fits(1):
        return 1
    parts = run_count_rule(raw, width)
    while parts <= PAL_MAX_PARTS and not fits(parts):
        parts *= 2
    return parts if parts <= PAL_MAX_PARTS else DIRECT


def layout(values, ftype, odd):
    """One integer field: alone at offset 0, or at offset 1 of an odd point_step behind a UINT8."""
    v = np.asarray(values).astype(_NP[ftype])
    if not odd:
        return cases.int_only(v, ftype)
    n = v.size
    info = cases.make_info([("p", 0, F.UINT8, None), ("value", 1, ftype, None)], 1 + v.dtype.itemsize + 2, n)
    return info, cases.pack(info, {"p": (np.arange(n) % 251).astype(np.uint8), "value": v}, n)


def _runs(flags):
    return M._run_lengths(flags)


def _value_runs(v):
    s = np.ones(v.size, bool)
    s[1:] = v[1:] != v[:-1]
    return s


def _delta_runs(v):
    d = v - np.concatenate([[0], v[:-1]]).astype(np.int64)
    s = np.ones(v.size, bool)
    s[1:] = d[1:] != d[:-1]
    return s


def _raw(v, ftype):
    return v.astype(_NP[ftype]).view(_NP[ftype]).astype(np.uint64) & np.uint64((1 << (8 * np.dtype(_NP[ftype]).itemsize)) - 1)


def crafted(ftype):
    """(name, int64-or-uint64 values before the cast to ftype, check(model column int64)) for one field type."""
    rs = np.random.RandomState(101 + int(ftype))
    bits = 8 * np.dtype(_NP[ftype]).itemsize
    wide = bits > 16
    out = []

    def add(name, v, check):
        out.append((name, np.asarray(v), check))

    # runs of 16384, 16383, 1 fill chunk 0 exactly; 127, 128, 5 follow in chunk 1
    lens = [16384, 16383, 1, 127, 128, 5]
    add("run_lengths", np.repeat(np.arange(len(lens)) * 37 + 11, lens),
        lambda v: (_runs(_value_runs(v[:CHUNK])).tolist() == lens[:3] and _runs(_value_runs(v[CHUNK:])).tolist() == lens[3:]))
    # one run covers chunk 0 and runs on into chunk 1: cut at 32768
    add("run_over_chunk_edge", np.concatenate([np.full(CHUNK + 1000, 77), np.full(500, 3)]),
        lambda v: (v[CHUNK - 1] == v[CHUNK] and _runs(_value_runs(v[:CHUNK])).tolist() == [CHUNK]))
    # runs of 64 that start one value in front of every wave edge (and so of every stage edge), values and deltas
    i = np.arange(3 * 1024 + 100)
    add("value_runs_straddle_every_wave", (i + 1) // 64,
        lambda v: all(v[e - 1] == v[e] for e in range(64, v.size, 64)))
    slopes = (np.arange(i.size // 64 + 2) % 7) + 1
    add("delta_runs_straddle_every_wave", np.cumsum(slopes[(i + 1) // 64]),
        lambda v: (lambda s: not s[64::64].any() and s[63::64].all())(_delta_runs(v)))
    # a constant delta across the chunk edge: chunk 1 restarts from prev = 0
    start, step = (5, 3) if wide else ((-16500, 1) if ftype == F.INT16 else (5, 1))  # (16 bits hold 32868 values at step 1)
    add("constant_delta_over_chunk_edge", start + step * np.arange(CHUNK + 100),
        lambda v: (_runs(_delta_runs(v[:CHUNK])).tolist() == [1, CHUNK - 1] and v[CHUNK] - v[CHUNK - 1] == step
                   and _runs(_delta_runs(v[CHUNK:])).tolist() == [1, 99]))
    for u in (1, 2, 3, 256, 257):
        add(f"unique_{u}", rs.permutation(1000) % u * 201 + 1, lambda v, u=u: np.unique(v).size == u)
    if wide:
        spread = (1 << 31) // 40000 if bits == 32 else (1 << 40)
        cap = PAL_CAP[bits // 8]
        for u, parts in ((cap, 1), (cap + 1, 2), (17500, 2 if bits == 32 else 4)):  # both sides of the table, a grown partition count
            v = (rs.permutation(u)[np.arange(u + 300) % u] + 1) * spread + 5
            add(f"unique_{u}", v, lambda v, u=u, parts=parts, t=ftype: (np.unique(v).size == u and partitions_needed(_raw(v, t), bits // 8) == parts))
        add("distinct_32768_with_zero", rs.permutation(CHUNK) * spread,
            lambda v, t=ftype: (np.unique(v).size == CHUNK and (v == 0).any() and partitions_needed(_raw(v, t), bits // 8) == (4 if bits == 32 else 8)))
        # The hash is no guarantee. Keys whose mix has an even low bit: the second attempt (2 partitions by the run count) puts
        # them all into partition 0 and overflows, the doubling branch separates them at 4. Keys whose mix agrees in its low 6
        # bits (64-bit fields: in its low 32 bits, all ones or all zeros, through the inverse mix): 64 partitions still
        # overflow and the direct count takes over.
        width = bits // 8
        pool = np.unique(rs.randint(1, 1 << 31, 1500000, dtype=np.int64)).astype(np.uint64)
        if bits == 64:
            pool = pool | (pool << np.uint64(33))
        even = rs.permutation(pool[mix(pool) & np.uint64(1) == 0])[:cap + cap // 6]
        add("skewed_partition", np.concatenate([even, even[:300]]),
            lambda v, t=ftype: run_count_rule(_raw(v, t), width) == 2 and partitions_needed(_raw(v, t), width) == 4)
        if bits == 32:
            same = [rs.permutation(pool[mix(pool) & np.uint64(63) == 63])[:cap + 60]]
        else:
            hi = rs.permutation(1 << 20)[:cap + 60].astype(np.uint64) << np.uint64(32)
            same = [unmix(hi | np.uint64(0xffffffff)), unmix(hi)]
        for k, keys in enumerate(same):
            add(f"hash_never_separates_{k}", np.concatenate([keys, keys[:300]]),
                lambda v, t=ftype, u=cap + 60: np.unique(v).size == u and partitions_needed(_raw(v, t), width) == DIRECT)
    else:
        add("distinct_32768", rs.permutation(CHUNK) * 2, lambda v: np.unique(v).size == CHUNK)
    if bits == 64:
        lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
        pat = np.array([lo, hi, lo, 0, lo, -1, hi, 1, lo + 1, hi - 1, 0, hi, hi, lo, lo], dtype=np.int64)
        add("int64_wrap_and_min", np.tile(pat, 20).view(np.uint64) if ftype == F.UINT64 else np.tile(pat, 20),
            lambda v: (lambda d: (d == lo).any() and (np.abs(v[1:].astype(float) - v[:-1].astype(float)) > 2.0 ** 63).any())(
                v - np.concatenate([[0], v[:-1]]).astype(np.int64)))
        # keys that differ only in their upper 32 bits, enough of them to share probe chains of the table
        add("upper_half_only", ((rs.permutation(4000)[np.arange(9000) % 4000].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | np.uint64(7),
            lambda v: (np.unique(v).size == 4000 and np.unique(v.view(np.uint64) & np.uint64(0xffffffff)).size == 1))
    # the probe is fooled: 4096 constant values, then noise, over two chunks
    noise = rs.randint(0, 1 << min(bits - 1, 40), 40000 - M.PROBE, dtype=np.int64)
    add("probe_fooled", np.concatenate([np.full(M.PROBE, 9), noise]), lambda v: True)
    return out


def all_crafted():
    """(id, info, data, values as the model sees them, check) for every type at an aligned and at an odd offset."""
    for ftype in TYPES:
        for name, values, check in crafted(ftype):
            for odd in (False, True):
                info, data = layout(values, ftype, odd)
                yield f"{ftype.name}_{'odd' if odd else 'aligned'}_{name}", info, data, check


def probe_fooled(ftype=F.UINT32, odd=False):
    values = [v for name, v, _c in crafted(ftype) if name == "probe_fooled"][0]
    return layout(values, ftype, odd)
