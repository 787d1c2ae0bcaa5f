"""A constructed voxel grid for every table branch of the viz pre-filter (viz_kernels.hip): GPU-free, shared by the CPU proofs of
tests/test_viz_grid_cases.py (every case reaches its branch in tests/viz_table_model.py; the oracle equals the compiled
reference on every cloud) and the GPU tests of tests/test_gpu_viz_grid.py (HIP against the oracle, byte for byte).

A Case is (name, family, step, xyz_off, res, [cloud bytes], cond). cond() asserts, in the model, the condition the case is
built for and returns the tags of the branches it has proven reached. No case holds more than 8192 points, except the two
batches of one-point clouds that make exactly 1024 and 1025 blocks. Nothing here is random: no fuzz seed range is consumed.

Bytes outside the x/y/z triple hold a pattern of the point's index in its cloud: two points of one voxel differ in their
bytes, so WHICH of them survived shows in the output."""
from collections import namedtuple

import numpy as np

import viz_table_model as M

Case = namedtuple("Case", "name family step off res clouds cond")

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
_NAN = np.uint32(0x7fc00000)
_box = []


def box():
    """[-80, 80)^3: 4 096 000 keys, about 2000 per LDS home (1024 with pairwise distinct homes in a 2048-slot table need that)."""
    if not _box:
        _box.append(M.KeyBox(-80, 80))
    return _box[0]


def wide_box():
    """[-512, 512)^2 x [-2, 2): for the 16384-slot table, whose home does not depend on z and on little of y."""
    if len(_box) < 2:
        box()
        _box.append(M.KeyBox((-512, -512, -2), (512, 512, 2)))
    return _box[1]


def cloud_of_bits(bits, step=16, off=0):
    """Cloud bytes from an (n, 3) uint32 array of float32 bit patterns (bit patterns: a NaN keeps its payload)."""
    bits = np.asarray(bits, dtype=np.uint32).reshape(-1, 3)
    n = len(bits)
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(step, dtype=np.uint64)[None, :]
    raw = (((i + 1) * 2654435761 + j * 40503) >> 9).astype(np.uint8)
    raw = np.ascontiguousarray(raw)
    raw[:, off:off + 12] = np.ascontiguousarray(bits).view(np.uint8).reshape(n, 12)
    return raw.reshape(-1)


def cloud_of_xyz(xyz, step=16, off=0):
    return cloud_of_bits(np.ascontiguousarray(xyz, dtype=np.float32).view(np.uint32).reshape(-1, 3), step, off)


def cloud_of_q(q, res=1.0, step=16, off=0, nan_at=()):
    """Integer voxel coordinates times a power-of-two resolution: exact in float32, lround(x * inv) gives q back."""
    xyz = (np.asarray(q, dtype=np.int64).reshape(-1, 3) * float(res)).astype(np.float32)
    bits = xyz.view(np.uint32).reshape(-1, 3).copy()
    if len(nan_at):
        bits[np.asarray(nan_at), 0] = _NAN
    return cloud_of_bits(bits, step, off)


def distinct_q(n, base=0):
    """n distinct small voxels (none of them the voxel (-70, -70, -70) that the cases use as THE voxel)."""
    i = np.arange(base, base + n, dtype=np.int64)
    return np.stack([i % 100 - 50, i // 100 % 100 - 50, i // 10000], axis=1)


def _survivors_are(case_name, clouds, step, off, res, want):
    for k, (c, w) in enumerate(zip(clouds, want)):
        got = M.survivors(c, step, off, res)
        assert np.array_equal(got, np.asarray(w, dtype=np.int64)), (case_name, k, got[:8], np.asarray(w)[:8])


# ---------------------------------------------------------------------------------------------------- a. sizes and keep patterns
def _pattern(n, pattern):
    """(q, nan_at, kept indexes) of an n-point cloud."""
    i = np.arange(n, dtype=np.int64)
    lane, wave, blk = i % 64, i // 64 % 16, i // 1024
    q = distinct_q(n)
    nan = np.zeros(n, dtype=bool)
    if pattern == "all":
        keep = np.ones(n, dtype=bool)
    elif pattern == "point0":
        q[:] = (-70, -70, -70)
        keep = i == 0
    elif pattern == "lane0":
        q = q[i - lane]                                          # every lane holds its wave's first voxel
        keep = lane == 0
    elif pattern == "lane63":
        nan = lane != 63
        keep = lane == 63
    elif pattern == "alternating":
        q = q[i - lane % 2]                                      # odd lanes repeat the even lane in front
        keep = lane % 2 == 0
    elif pattern.startswith("wave"):
        keep = wave == int(pattern[4:])
        nan = ~keep
    elif pattern == "nan_but_last":
        nan = i != n - 1
        keep = ~nan
    elif pattern == "last_block":
        nan = blk != (n - 1) // 1024
        keep = ~nan
    else:
        raise ValueError(pattern)
    return q, np.flatnonzero(nan), np.flatnonzero(keep)


PATTERNS = ["all", "point0", "lane0", "lane63", "alternating", "wave0", "wave7", "wave15", "nan_but_last", "last_block"]
_SIZE_GROUPS = [[1, 63, 64, 65, 1023, 1024, 1025], [2047, 2048, 2049], [3073]]


def family_a():
    out = []
    for pattern in PATTERNS:
        for g, sizes in enumerate(_SIZE_GROUPS):
            built = [_pattern(n, pattern) for n in sizes]
            clouds = [cloud_of_q(q, nan_at=nan) for q, nan, _ in built]
            want = [keep for _, _, keep in built]
            name = f"a/{pattern}/sizes{g}"

            def cond(name=name, clouds=clouds, want=want, pattern=pattern):
                _survivors_are(name, clouds, 16, 0, 1.0, want)
                return {"keep:" + pattern}
            out.append(Case(name, "a", 16, 0, 1.0, clouds, cond))
    return out


# ---------------------------------------------------------------------------------------------------- b. LDS chains
LDS_M = [2, 3, 16, 64, 256, 1024]
LDS_S = [0, 1000, 2040, 2047]


def _lds_block(m, s, variant):
    """(q of the cloud, kept indexes). plain: the m keys. same_wave: key k at 2k and 2k + 1. later_wave: the m keys, then
    (from the next wave boundary on) the m keys again. A full block (m = 1024) has no room for repeats: they make a second
    block, which then keeps nothing (next_block)."""
    n = {"plain": m, "same_wave": 2 * m, "later_wave": -(-m // 64) * 64 + m, "next_block": 2 * m}[variant]
    idx = box().same_lds(s, m, cap=M.capacity(n))
    q = box().q[idx]
    if variant == "plain":
        return q, np.arange(m)
    if variant == "same_wave":
        return np.repeat(q, 2, axis=0), np.arange(m) * 2
    if variant == "next_block":
        return np.concatenate([q, q[::-1]]), np.arange(m)
    pad = -(-m // 64) * 64 - m                                   # copies of key 0 up to the wave boundary
    return np.concatenate([q, np.repeat(q[:1], pad, axis=0), q]), np.arange(m)


def family_b():
    out = []
    for m in LDS_M:
        for s in LDS_S:
            for variant in ("plain", "same_wave", "later_wave") if m < 1024 else ("plain", "next_block"):
                q, keep = _lds_block(m, s, variant)
                cloud = cloud_of_q(q)
                name = f"b/m{m}/s{s}/{variant}"

                def cond(name=name, cloud=cloud, q=q, keep=keep, m=m, s=s, variant=variant):
                    keys = M.key_of_q(q)
                    first = keys[:1024]
                    assert np.unique(first).size == m and np.all(M.lds_home(first) == s), name
                    wraps, chain, occ = M.lds_facts(first)
                    assert chain == m and occ.sum() == m, name   # slots s .. s + m - 1 (mod 2048): the last key walks m - 1
                    assert wraps == (m > M.LDS_SLOTS - s), name
                    cap = M.capacity(len(q))
                    assert np.unique(M.hbm_home(np.unique(keys), cap)).size == m, (name, "HBM homes are pairwise distinct")
                    if variant == "later_wave":
                        assert np.all((np.arange(len(q))[-m:] // 64) > (np.arange(m) // 64)), name
                    _survivors_are(name, [cloud], 16, 0, 1.0, [keep])
                    return {"lds_chain"} | ({"lds_wrap"} if wraps else set())
                out.append(Case(name, "b", 16, 0, 1.0, [cloud], cond))
    return out


# ---------------------------------------------------------------------------------------------------- c. HBM chains
HBM_JM = [(j, m) for j in (0, 1, 3) for m in (2, 8, 32) if m > j + 1]
HBM_N = [300, 1000, 2000, 8192]                                  # caps 1024, 2048, 4096, 16384


def hbm_cloud(n, j, m, every_block=False):
    """n points: m keys whose HBM home is slot cap - 1 - j (LDS homes pairwise distinct), the rest plain distinct voxels.
    Colliding key k stands in block k % n_blocks (at thread 7 + 9 (k // n_blocks)); with every_block once in EVERY block
    (the same thread in each). Returns (q, positions of the colliding points [copy][key])."""
    cap = M.capacity(n)
    nb = -(-n // 1024)
    q = distinct_q(n)
    kb = box() if cap <= 4096 else wide_box()
    coll = kb.q[kb.same_hbm(cap, cap - 1 - j, m + 8)]
    coll = coll[~np.isin(M.key_of_q(coll), M.key_of_q(q))][:m]   # (none of the plain voxels)
    assert len(coll) == m
    if every_block:
        pos = np.array([[b * 1024 + 5 + 7 * k for k in range(m)] for b in range(nb)])
    else:
        pos = np.array([[(k % nb) * 1024 + 7 + 9 * (k // nb) for k in range(m)]])
    assert pos.max() < n
    for row in pos:
        q[row] = coll
    return q, pos


def family_c():
    out = []
    for n in HBM_N:
        nb = -(-n // 1024)
        for j, m in HBM_JM:
            for every_block in ([False, True] if nb > 1 else [False]):
                q, pos = hbm_cloud(n, j, m, every_block)
                cloud = cloud_of_q(q)
                name = f"c/n{n}/j{j}/m{m}/" + ("every_block" if every_block else "spread")

                def cond(name=name, cloud=cloud, q=q, pos=pos, n=n, j=j, m=m, nb=nb, every_block=every_block):
                    cap, wraps, chain, occ, sent, inserts = M.hbm_facts(cloud, 16, 0, 1.0)
                    keys = M.key_of_q(q)
                    coll = keys[pos[0]]
                    assert cap == M.capacity(n) and np.all(M.hbm_home(coll, cap) == cap - 1 - j), name
                    assert np.unique(M.lds_home(coll)).size == m, (name, "only the HBM probe chains")
                    assert wraps and M.chain_bound(cap - 1 - j, occ) >= m and occ[0], name
                    times = inserts[np.searchsorted(sent, np.sort(coll))]
                    assert np.all(times == (nb if every_block else 1)), name
                    blocks_of = set((pos[0] // 1024).tolist())
                    want = np.ones(n, dtype=bool)
                    want[pos[1:].reshape(-1)] = False
                    _survivors_are(name, [cloud], 16, 0, 1.0, [np.flatnonzero(want)])
                    tags = {f"hbm_wrap:{cap}"}
                    if every_block:
                        tags.add("cas_same_key")
                    if len(blocks_of) > 1:
                        tags.add("cas_other_key")
                    return tags
                out.append(Case(name, "c", 16, 0, 1.0, [cloud], cond))
    return out


# ---------------------------------------------------------------------------------------------------- d. first occurrence across blocks
_V = (-70, -70, -70)


def _with_voxel_at(n, at):
    q = distinct_q(n)
    q[np.asarray(at)] = _V
    return q


def family_d():
    n = 8192
    sets = [("every_block", [[b * 1024 + (37 * b + 11) % 1024 for b in range(8)]]),
            ("boundary", [[b * 1024 + 1023, (b + 1) * 1024] for b in range(7)]),
            ("many_in_5_one_high_in_0", [[1000] + list(range(5 * 1024 + 100, 5 * 1024 + 600))]),
            ("last_block_only", [[7 * 1024 + 3, 7 * 1024 + 500, 8191]])]
    out = []
    for label, ats in sets:
        if label == "boundary":                                  # seven clouds of 8192 points: one case each
            groups = [(f"d/boundary/b{b}", [at]) for b, at in enumerate(ats)]
        else:
            groups = [("d/" + label, ats)]
        for name, group in groups:
            clouds = [cloud_of_q(_with_voxel_at(n, at)) for at in group]

            def cond(name=name, clouds=clouds, group=group):
                want = []
                for at in group:
                    keep = np.ones(n, dtype=bool)
                    keep[np.asarray(at)[1:]] = False
                    assert at[0] == min(at)
                    want.append(np.flatnonzero(keep))
                _survivors_are(name, clouds, 16, 0, 1.0, want)
                return {"first_across_blocks"}
            out.append(Case(name, "d", 16, 0, 1.0, clouds, cond))
    q0 = distinct_q(1024)
    q = np.concatenate([q0] + [q0[(np.arange(1024) * (2 * b + 1) + 5 * b) % 1024] for b in range(1, 8)])
    cloud = cloud_of_q(q)

    def cond_copies(cloud=cloud):
        _survivors_are("d/copies_of_block_0", [cloud], 16, 0, 1.0, [np.arange(1024)])
        firsts = M.block_firsts(M.key_of_q(q), np.ones(len(q), dtype=bool))
        assert all(len(f) == 1024 for f in firsts)               # every block sends all of its points to the HBM table
        return {"first_across_blocks", "blocks_keep_nothing"}
    out.append(Case("d/copies_of_block_0", "d", 16, 0, 1.0, [cloud], cond_copies))
    return out


# ---------------------------------------------------------------------------------------------------- e. key edges
def _f32(v):
    return np.float32(v)


def family_e():
    """Pairs (alias, plain) per axis: [alias, plain] in one row of voxels, [plain, alias] in another -- the alias decides
    which of the two survives. The other two axes carry the row number."""
    T20, T21 = 2.0 ** 20, 2.0 ** 21
    pairs = [(-T20 - 1, T20 - 1), (T20, -T20), (5 + T21, 5.0), (5 - T21, 5.0), (-T20 + T21, -T20), (T20 - 1 - T21, T20 - 1),
             (2.0 ** 31, 0.0), (-2.0 ** 31 - 2.0 ** 8, -256.0), (2.0 ** 32 + 512 * 3, 1536.0), (2.0 ** 32 + 512, 512.0),
             (2.0 ** 63, 0.0), (-2.0 ** 63, 0.0)]
    rows, want, row = [], [], 0
    for a in range(3):
        for alias, plain in pairs:
            for order in ((alias, plain), (plain, alias)):
                for v in order:
                    p = [float(row + 3), float(-row - 3), float(row + 3)]
                    p[a] = v
                    rows.append(p)
                want += [len(rows) - 2]
                row += 1
    # not aliases: half the field's range apart (and a quarter) is another voxel -- a mask one bit short would merge them
    near_at = len(rows)
    for a in range(3):
        for v in (5.0, 5 - T20, 5 + 2.0 ** 19, 5 - 2.0 ** 19):
            p = [float(row + 3), float(-row - 3), float(row + 3)]
            p[a] = v
            rows.append(p)
            want.append(len(rows) - 1)
        row += 1
    # whole keys: 0 and 2^63 - 1 (all ones in 63 bits: not the free marker of either table), each twice
    lo, hi = [-T20] * 3, [T20 - 1] * 3
    whole_at = len(rows)
    rows += [lo, hi, hi, lo]
    want += [whole_at, whole_at + 1]
    xyz = np.array(rows, dtype=np.float32)
    assert np.array_equal(xyz.astype(np.float64), np.array(rows))  # every value is a float32
    cloud = cloud_of_xyz(xyz)

    def cond():
        k = M.key(xyz, 1.0)
        for g in range(0, near_at, 2):
            assert k[g] == k[g + 1] and not np.array_equal(xyz[g], xyz[g + 1]), ("e/edges", g)
        assert np.unique(k[near_at:whole_at]).size == 12
        assert int(k[whole_at]) == 0 and int(k[whole_at + 1]) == (1 << 63) - 1
        assert np.all(M.field(M.quant(np.float32([-T20, T20 - 1]), 1.0)) == np.array([0, M.FIELD], dtype=np.uint64))
        _survivors_are("e/edges", [cloud], 16, 0, 1.0, [want])
        return {"alias", "near_alias_distinct", "key_zero", "key_all_ones"}
    out = [Case("e/edges", "e", 16, 0, 1.0, [cloud], cond)]
    # a finite input whose float32 product is infinite: lround gives LONG_MIN, the low 32 bits are 0 -- the voxel of 0.0
    inf_rows, inf_want = [], []
    for a in range(3):
        for order in ((3.4e38, 0.0), (0.0, -3.4e38), (-3.4e38, 3.4e38)):
            for v in order:
                p = [0.001 * (len(inf_want) + 3)] * 3
                p[a] = v
                inf_rows.append(p)
            inf_want.append(len(inf_rows) - 2)
    ixyz = np.array(inf_rows, dtype=np.float32)
    icloud = cloud_of_xyz(ixyz)

    def cond_inf():
        with np.errstate(over="ignore"):
            t = ixyz * (np.float32(1) / np.float32(0.001))
        assert np.isinf(t).sum() == 12 and np.all(np.isfinite(ixyz))
        assert np.all(M.quant(np.float32([3.4e38, -3.4e38]), 0.001) == M.INT64_MIN)
        _survivors_are("e/infinite_product", [icloud], 16, 0, 0.001, [inf_want])
        return {"alias", "infinite_product"}
    out.append(Case("e/infinite_product", "e", 16, 0, 0.001, [icloud], cond_inf))
    return out


# ---------------------------------------------------------------------------------------------------- f. rounding
def float32_only_ties(res=0.001, k_max=200_000):
    """float32 values whose float32 product with 1 / res is exactly k + 0.5 while the exact product is not: the floats nearest
    (k + 0.5) * res and their two neighbours, k < k_max. Returns (values, float32 products)."""
    inv = np.float32(1) / np.float32(res)
    c = (np.arange(k_max).astype(np.float32) + np.float32(0.5)) * np.float32(res)
    v = np.concatenate([np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))])
    t = (v * inv).astype(np.float32).astype(np.float64)
    exact = v.astype(np.float64) * float(inv)                    # 24 x 24 bits: exact in float64
    tie = (t - np.floor(t) == 0.5) & (exact != t)
    return v[tie], t[tie]


def _triples(values, res):
    """Per value v, on axis g % 3: [partner in v's voxel, v, partner in the neighbouring voxel the product lies towards]
    and the reverse order. Correct rounding keeps points 0 and 2 of the first and 0 and 1 of the second triple; rounding v
    into the neighbour keeps 0 and 1, and 0 and 2. Returns (xyz, kept indexes, (value, its voxel, the neighbour) per triple)."""
    inv = np.float32(1) / np.float32(res)
    rows, want, info = [], [], []
    for g, v in enumerate(values):
        v = np.float32(v)
        t = float(np.float32(v * inv))
        qc = int(M.quant(v, res))
        lo, hi = int(np.floor(t)), int(np.ceil(t))
        assert lo != hi, (v, res, "the product is an integer: no rounding to test")
        qw = lo if qc == hi else hi
        pc, pw = np.float32(qc * float(res)), np.float32(qw * float(res))
        if qc == 0:
            pc = np.float32(0.0)
        for order, kept in (((pc, v, pw), (0, 2)), ((pw, v, pc), (0, 1))):
            other = np.float32((3 + len(want) // 2) * 4 * float(res))
            for x in order:
                p = [other, other, other]
                p[g % 3] = x
                rows.append(p)
            want += [len(rows) - 3 + kept[0], len(rows) - 3 + kept[1]]
            info.append((v, qc, qw, pc, pw))
    return np.array(rows, dtype=np.float32), want, info


def _tie_values(res, ks=(0, 1, 2, 7, 1000)):
    out = []
    for k in ks:
        for sign in (1.0, -1.0):
            c = np.float32(sign * (k + 0.5) * res)
            out += [c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(sign * np.inf))]
    return out


def family_f():
    out = []
    FLT_MIN, DEN = np.float32(1.17549435e-38), np.float32(1e-45)
    sets = [("exact_ties/res1.0", 1.0, _tie_values(1.0)), ("exact_ties/res0.25", 0.25, _tie_values(0.25))]
    for res in (0.001, 0.01, 0.05):
        sets.append((f"nearest_ties/res{res}", res, _tie_values(res)))
    for res in (1.0, 0.001):
        sets.append((f"tiny/res{res}", res, [DEN, -DEN, FLT_MIN, -FLT_MIN, np.float32(FLT_MIN / 2), np.float32(-FLT_MIN / 2)]))
    tv, tt = float32_only_ties()
    pick = tv[np.linspace(0, len(tv) - 1, 48).astype(int)]       # each with its neighbour on either side, like the ties above
    only32 = np.stack([pick, np.nextafter(pick, np.float32(0)), np.nextafter(pick, np.float32(np.inf))], axis=1).reshape(-1)
    sets.append(("float32_only_ties/res0.001", 0.001, list(only32)))
    for label, res, values in sets:
        xyz, want, info = _triples(values, res)
        cloud = cloud_of_xyz(xyz)
        name = "f/" + label

        def cond(name=name, xyz=xyz, want=want, info=info, res=res, cloud=cloud, label=label):
            inv = np.float32(1) / np.float32(res)
            for v, qc, qw, pc, pw in info:
                assert int(M.quant(pc, res)) == qc and int(M.quant(pw, res)) == qw and abs(qc - qw) == 1, (name, v)
            tags = {"rounding"}
            if label.startswith("exact_ties"):
                t = np.array([float(np.float32(i[0] * inv)) for i in info[::6]])      # the ties themselves
                assert np.all(np.abs(t) % 1.0 == 0.5) and all(abs(i[1]) == abs(i[2]) + 1 for i in info[::6]), name
                tags.add("exact_tie")
            if label.startswith("float32_only"):
                for v, qc, qw, _pc, _pw in info[::6]:
                    t = float(np.float32(v * inv))
                    exact = float(v) * float(inv)
                    assert abs(t) % 1.0 == 0.5 and exact != t, (name, v)
                    # a double-precision (or fused) product rounds where the exact product lies
                    assert int(np.trunc(exact + np.copysign(0.5, exact))) in (qc, qw)
                tags.add("float32_only_tie")
                if any(int(np.trunc(float(i[0]) * float(inv) + 0.5)) == i[2] for i in info[::6]):
                    tags.add("double_product_differs")
            _survivors_are(name, [cloud], 16, 0, res, [want])
            return tags
        out.append(Case(name, "f", 16, 0, res, [cloud], cond))
    # -0.0 against +0.0: one voxel, different bytes, the first wins -- in both orders, on every axis
    z = []
    for a in range(3):
        for first, second in ((0.0, -0.0), (-0.0, 0.0)):
            for v in (first, second):
                p = [float(len(z) // 2 + 2)] * 3
                p[a] = v
                z.append(p)
    zxyz = np.array(z, dtype=np.float32)
    zcloud = cloud_of_xyz(zxyz)

    def cond_zero():
        bits = zxyz.view(np.uint32).reshape(-1, 3)
        assert (bits == 0x80000000).sum() == 6
        _survivors_are("f/signed_zero", [zcloud], 16, 0, 1.0, [np.arange(0, len(z), 2)])
        return {"signed_zero"}
    out.append(Case("f/signed_zero", "f", 16, 0, 1.0, [zcloud], cond_zero))
    return out


# ---------------------------------------------------------------------------------------------------- g. non-finite
NONFINITE = [0x7fc00000, 0x7fa00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000]
FLT_MAX_BITS = [0x7f7fffff, 0xff7fffff]


def family_g():
    rows, dropped = [], []
    for a in range(3):
        for b in NONFINITE + FLT_MAX_BITS:
            plain = np.array([len(rows) + 2.0] * 3, dtype=np.float32).view(np.uint32)
            rows.append(plain.copy())                            # a plain point of the same row in front ...
            bad = plain.copy()
            bad[a] = b
            rows.append(bad)
            if b in NONFINITE:
                dropped.append(len(rows) - 1)
            rows.append(plain.copy() + np.uint32(1 << 23))       # ... and another voxel behind (the value doubled)
    bits = np.array(rows, dtype=np.uint32)
    cloud = cloud_of_bits(bits)

    def cond():
        fin = M.finite(bits.view(np.float32))
        assert np.array_equal(np.flatnonzero(~fin), dropped) and len(dropped) == 21
        keep = np.ones(len(bits), dtype=bool)
        keep[dropped] = False
        _survivors_are("g/per_axis", [cloud], 16, 0, 1.0, [np.flatnonzero(keep)])
        assert np.array_equal(cloud.reshape(-1, 16)[:, :12].copy().view(np.uint32), bits)     # payloads intact
        return {"nonfinite", "flt_max_kept"}
    return [Case("g/per_axis", "g", 16, 0, 1.0, [cloud], cond)]


# ---------------------------------------------------------------------------------------------------- h. copy and load branches
LAYOUTS = [(12, 0), (16, 0), (16, 4), (20, 8), (32, 0), (48, 16), (13, 1), (18, 0), (19, 3)]
MISALIGN = [0, 4, 1]


def family_h():
    """1100 points (two blocks): every third point repeats the one in front, two NaN points. Run device resident at every
    (input, output) misalignment of MISALIGN; the branch of every survivor follows from the addresses."""
    n = 1100
    q = distinct_q(n)
    q[2::3] = q[1::3][: len(q[2::3])]
    out = []
    for step, off in LAYOUTS:
        cloud = cloud_of_q(q, step=step, off=off, nan_at=[0, 1027])
        name = f"h/step{step}/off{off}"

        def cond(name=name, cloud=cloud, step=step, off=off):
            kept = M.survivors(cloud, step, off, 1.0)
            assert 0 < len(kept) < n and kept[0] == 1
            tags = set()
            for mi in MISALIGN:
                for mo in MISALIGN:
                    br = {M.copy_branch(step, mi + int(i) * step, mo + r * step) for r, i in enumerate(kept)}
                    tags |= {"copy:" + b for b in br}
                    if step in (16, 32) and (mi, mo) == (0, 0):
                        assert br == {"uint4"}, name
                    if step in (16, 32) and (mi, mo) == (0, 4):
                        assert br == {"dword"}, name
                        tags.add("uint4_to_dword_by_output")
                    if step in (16, 32) and (mi, mo) == (4, 0):
                        assert br == {"dword"}, name
                        tags.add("uint4_to_dword_by_input")
                tags |= {"load:" + M.load_branch(int(r)) for r in np.unique((mi + np.arange(n) * step + off) % 4)}
            return tags
        out.append(Case(name, "h", step, off, 1.0, [cloud], cond))
    return out


# ---------------------------------------------------------------------------------------------------- i. batches
def _first_slots_cloud(n, slots=4):
    """n points whose table (capacity(n)) has its first `slots` slots occupied by keys that HOME there."""
    cap = M.capacity(n)
    q = distinct_q(n)
    used = set()
    for s in range(slots):
        pick = box().q[box().same_hbm(cap, s, 1, exclude_lds=used)]
        used.add(int(M.lds_home(M.key_of_q(pick))[0]))
        q[11 + 50 * s] = pick[0]
    return q


def family_i():
    zero = np.zeros(0, np.uint8)
    wrap300 = cloud_of_q(hbm_cloud(300, 0, 8)[0])                # cap 1024, a chain of 8 from slot 1023
    wrap2000 = cloud_of_q(hbm_cloud(2000, 1, 32, every_block=True)[0])
    wrap8192 = cloud_of_q(hbm_cloud(8192, 3, 32)[0])
    live300, live2000 = cloud_of_q(_first_slots_cloud(300)), cloud_of_q(_first_slots_cloud(2000))
    lds = cloud_of_q(_lds_block(64, 2047, "later_wave")[0])
    every = cloud_of_q(_with_voxel_at(8192, [b * 1024 + (37 * b + 11) % 1024 for b in range(8)]))
    cross = cloud_of_q(_with_voxel_at(3072, [1023, 1024, 2500]))  # (a three-block cloud: family d's boundary pair in a batch)
    one = [cloud_of_q(distinct_q(1, base=k % 3), nan_at=[0] if k % 7 == 3 else []) for k in range(1025)]
    batches = [("wrap_before_live_entries", [live300, wrap300, live300, wrap2000, live2000, wrap300, live2000], "wrap"),
               ("same_collision_cloud_twice", [wrap300, wrap300.copy(), wrap2000, wrap2000.copy(), lds, lds.copy()], "twice"),
               ("zero_point_clouds", [zero, lds, zero, zero, zero, wrap300, cross, zero], "zeros"),
               ("eight_block_chain", [wrap8192], "big"), ("eight_block_first", [zero, every, zero], "big"),
               ("blocks1024", one[:1024], "blocks"), ("blocks1025", one[:1025], "blocks")]
    out = []
    for label, clouds, kind in batches:
        for rev in (False, True):
            cl = clouds[::-1] if rev else clouds
            name = f"i/{label}" + ("/reversed" if rev else "")

            def cond(name=name, cl=cl, kind=kind, label=label):
                n = [c.size // 16 for c in cl]
                tags = {"batch"}
                if kind == "wrap":
                    hit = 0
                    for k in range(len(cl) - 1):
                        _cap, wraps, _chain, _occ, _s, _i = M.hbm_facts(cl[k], 16, 0, 1.0)
                        nxt = M.hbm_facts(cl[k + 1], 16, 0, 1.0)[3]
                        if wraps and nxt[:4].all():
                            hit += 1                             # a probe that ran on instead of wrapping lands in live entries
                    assert hit >= 2, name
                    tags.add("wrap_before_live_entries")
                elif kind == "twice":
                    assert sum(bool(a.size) and np.array_equal(a, b) for a, b in zip(cl, cl[1:])) == 3, name
                    tags.add("same_cloud_twice")
                elif kind == "zeros":
                    z = [m == 0 for m in n]
                    assert z[0] and z[-1] and any(z[k] and z[k + 1] and z[k + 2] for k in range(len(z) - 2)), name
                    tags.add("zero_point_clouds")
                elif kind == "blocks":
                    assert set(n) == {1} and len(cl) == int(label[6:]), name
                    tags.add(label)
                return tags
            out.append(Case(name, "i", 16, 0, 1.0, cl, cond))
    return out


# ---------------------------------------------------------------------------------------------------- the grid
FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g,
            "h": family_h, "i": family_i}
_grid = {}


def family(f):
    if f not in _grid:
        _grid[f] = FAMILIES[f]()
    return _grid[f]


def grid():
    return [c for f in FAMILIES for c in family(f)]


# every tag the grid has to reach (tests/test_viz_grid_cases.py::test_branches_reached_over_the_whole_grid)
REQUIRED = ({"keep:" + p for p in PATTERNS} | {"lds_chain", "lds_wrap", "cas_other_key", "cas_same_key", "first_across_blocks",
            "blocks_keep_nothing", "alias", "near_alias_distinct", "key_zero", "key_all_ones", "infinite_product", "rounding", "exact_tie",
            "float32_only_tie", "double_product_differs", "signed_zero", "nonfinite", "flt_max_kept", "copy:uint4", "copy:dword",
            "copy:byte", "load:aligned", "load:bytes", "uint4_to_dword_by_output", "uint4_to_dword_by_input", "batch",
            "wrap_before_live_entries", "same_cloud_twice", "zero_point_clouds", "blocks1024", "blocks1025"}
            | {f"hbm_wrap:{M.capacity(n)}" for n in HBM_N})
