"""The constructed grid of the viz pre-filter (tests/viz_grid_cases.py) on the CPU: every case reaches the branch it is built
for in the numpy model of the kernels' tables (tests/viz_table_model.py), the C oracle equals the compiled reference on every
cloud of the grid, the model's survivors equal the oracle's, and the branches reached over the whole grid are counted. The
lines of viz_kernels.hip that no mutant may touch on a shared GPU (the wrap masks, the free-slot compares) are held by these
reachability proofs."""
import numpy as np
import pytest

import cases
import viz_grid_cases as G
import viz_table_model as M
from cloudini_amd.schema import FieldType as F

FAMS = list(G.FAMILIES)


def _info(case, n):
    off, res = case.off, case.res
    return cases.make_info([("x", off, F.FLOAT32, res), ("y", off + 4, F.FLOAT32, res), ("z", off + 8, F.FLOAT32, res)], case.step, n)


# ---------------------------------------------------------------------------------------------------- the model itself
def test_model_key_restates_the_kernel():
    q = np.array([[0, 0, 0], [-(1 << 20), (1 << 20) - 1, 5], [1 << 20, -(1 << 20) - 1, 5 + (1 << 21)]], dtype=np.int64)
    k = M.key_of_q(q)
    assert int(k[0]) == (1 << 20) | (1 << 41) | (1 << 62)
    assert int(k[1]) == 0 | (M.FIELD << 21) | (((1 << 20) + 5) << 42) and k[1] == k[2]
    assert np.array_equal(M.key(q.astype(np.float32), 1.0), k) and np.array_equal(M.key(q.astype(np.float32) * 0.25, 0.25), k)
    # half away from zero, in the float32 product; outside int64 -> INT64_MIN (low 32 bits 0)
    assert M.quant(np.float32([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997]), 1.0).tolist() == [1, -1, 2, 3, -3, 0]
    assert M.quant(np.float32([2.0 ** 63, -2.0 ** 63, 3.4e38, 2.0 ** 62]), 1.0).tolist() == [M.INT64_MIN, M.INT64_MIN, M.INT64_MIN, 1 << 62]
    assert int(M.hash_(np.uint64(3))) == (3 * 0x9E3779B97F4A7C15) % (1 << 64)
    h = int(M.hash_(k[1]))
    assert int(M.lds_home(k[1])) == (h >> 40) & 2047 and int(M.hbm_home(k[1], 4096)) == (h >> 20) & 4095
    assert [M.capacity(n) for n in (0, 1, 512, 513, 1024, 1025, 2048, 2049, 8192)] == [1024, 1024, 1024, 2048, 2048, 4096, 4096, 8192, 16384]
    assert M.blocks(2049) == [(0, 1024), (1024, 2048), (2048, 2049)] and M.blocks(0) == []


def test_model_tables_do_not_depend_on_the_insertion_order():
    rs = np.random.RandomState(1)
    homes = np.concatenate([rs.randint(0, 64, 40), [61, 62, 63, 63, 63]])
    occ = M.occupied(homes, 64)
    for _ in range(20):
        assert np.array_equal(M.occupied(rs.permutation(homes), 64), occ)
    assert occ.sum() == len(homes)
    assert M.stored_past_the_wrap([63, 63], 64) and M.stored_past_the_wrap([60, 61, 62, 63, 62], 64)
    assert not M.stored_past_the_wrap([63, 0, 1], 64) and not M.stored_past_the_wrap([62, 62], 64)
    assert M.chain_bound(62, M.occupied([62, 62, 62], 64)) == 3 and M.occupied([62, 62, 62], 64)[0]
    assert [M.copy_branch(*a) for a in ((16, 32, 64), (16, 32, 68), (16, 36, 64), (12, 0, 0), (32, 1, 0), (18, 0, 0), (20, 4, 8))] == \
        ["uint4", "dword", "dword", "dword", "byte", "byte", "dword"]


def test_key_picker_census():
    """What the issue measured on [-64, 64)^3 at res 1.0, and that q * res comes back as q for the power-of-two resolutions."""
    box = M.keys_in_box(-64, 64)
    assert len(box.keys) == 2_097_152 and np.unique(box.keys).size == len(box.keys)
    assert np.bincount(box.lds, minlength=2048).min() >= 1013
    for cap, least in ((1024, 1792), (2048, 768), (4096, 256)):
        assert np.bincount(M.hbm_home(box.keys, cap), minlength=cap).min() >= least, cap
    both = np.unique(box.lds * 1024 + M.hbm_home(box.keys, 1024), return_counts=True)[1]
    assert both.max() <= 6
    idx = box.same_both(1024, 3)
    assert np.unique(box.lds[idx]).size == 1 and np.unique(M.hbm_home(box.keys[idx], 1024)).size == 1
    for res in (1.0, 0.25):
        xyz = (box.q[::97] * res).astype(np.float32)
        assert np.array_equal(xyz.astype(np.float64), box.q[::97] * res) and np.array_equal(M.key(xyz, res), box.keys[::97])
    idx = box.same_hbm(2048, 2047, 8)
    assert np.unique(box.lds[idx]).size == 8 and np.all(M.hbm_home(box.keys[idx], 2048) == 2047)


def test_float32_only_ties_census():
    """201 652 values for k < 200 000 at res 0.001: a tie in the float32 product, none in the exact product."""
    v, t = G.float32_only_ties()
    assert len(v) == 201_652 and np.all(t - np.floor(t) == 0.5)


# ---------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("fam", FAMS)
def test_every_case_meets_its_condition_in_the_model(fam):
    for case in G.family(fam):
        tags = case.cond()
        assert tags, case.name
        assert sum(c.size // case.step for c in case.clouds) <= 8192 or case.name.startswith("i/blocks10"), case.name
        assert all(c.dtype == np.uint8 and c.size % case.step == 0 for c in case.clouds), case.name


@pytest.mark.parametrize("fam", FAMS)
def test_model_survivors_equal_the_oracle(oracle, fam):
    seen = set()
    for case in G.family(fam):
        for k, c in enumerate(case.clouds):
            if c.tobytes() in seen:
                continue
            seen.add(c.tobytes())
            want = oracle.viz_preprocess(c, case.step, case.off, case.res)
            assert np.array_equal(M.survivor_bytes(c, case.step, case.off, case.res), want), (case.name, k)


@pytest.mark.parametrize("fam", FAMS)
def test_oracle_equals_the_reference_on_every_cloud(oracle, reflib, fam):
    seen = set()
    for case in G.family(fam):
        for k, c in enumerate(case.clouds):
            if c.size == 0 or c.tobytes() in seen:
                continue
            seen.add(c.tobytes())
            ref = reflib.viz_preprocess(_info(case, c.size // case.step), c)[0]
            assert np.array_equal(oracle.viz_preprocess(c, case.step, case.off, case.res), ref), (case.name, k)


def test_branches_reached_over_the_whole_grid():
    """How often each branch is proven reached (cases per tag). The floor per tag is what the grid is built to have."""
    count = {}
    for case in G.grid():
        for t in case.cond():
            count[t] = count.get(t, 0) + 1
    print(sorted(count.items()))
    assert G.REQUIRED <= set(count), sorted(G.REQUIRED - set(count))
    assert count["lds_wrap"] == 28 and count["lds_chain"] == 68          # m > 2048 - s: 5 + 2 + ... of the 68 blocks
    for cap in (1024, 2048):
        assert count[f"hbm_wrap:{cap}"] == len(G.HBM_JM)
    for cap in (4096, 16384):
        assert count[f"hbm_wrap:{cap}"] == 2 * len(G.HBM_JM)
    assert count["cas_other_key"] == 2 * len(G.HBM_JM) == count["cas_same_key"]
    for p in G.PATTERNS:
        assert count["keep:" + p] == 3
    for b in ("uint4", "dword", "byte"):
        assert count["copy:" + b] >= 3
    assert count["load:bytes"] >= 3 and count["load:aligned"] == len(G.LAYOUTS)
    assert count["uint4_to_dword_by_output"] == 3 == count["uint4_to_dword_by_input"]     # steps 16 (two offsets) and 32


def test_cases_for_the_gather_prefix_mutant_stay_inside_the_output():
    """`lane <= wave` in the gather prefix adds a wave's own count to its rank. Where this holds the shifted ranks stay inside
    the output capacity (every input point has room there), so that mutant may run: family a's 'alternating' clouds."""
    for case in G.family("a"):
        if "/alternating/" not in case.name:
            continue
        waves, total = [], 0
        for c in case.clouds:
            n = c.size // 16
            keep = np.zeros(n, dtype=bool)
            keep[M.survivors(c, 16, 0, 1.0)] = True
            for lo, hi in M.blocks(n):
                waves.append([int(keep[w:min(w + 64, hi)].sum()) for w in range(lo, hi, 64)])
            total += n
        assert M.ranks_shifted_stay_inside(waves, total), case.name
