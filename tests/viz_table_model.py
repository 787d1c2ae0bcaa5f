"""What decides a point's fate in viz_kernels.hip, restated in numpy (no GPU): the voxel key, the two hash tables of
k_viz_insert (2048 LDS slots per 1024-point block, `capacity(n)` HBM slots per cloud, both open addressing with wrap-around),
the block cut, first occurrences, the copy branch of k_viz_gather.

The model is used ONLY to prove that a constructed case (tests/viz_grid_cases.py) reaches the branch it is built for. Expected
bytes are always the C oracle's (oracle.viz_preprocess), never the model's; tests/test_viz_grid_cases.py holds the model's
`survivors` against the oracle as a check on the model.

Everything derived from a table here holds in EVERY execution order: the set of occupied slots of a linear-probing table does
not depend on the order of the inserts, so "the distance from a key's home to the first free slot of the final table" bounds
the chain it walks, and "more distinct keys home in the last a slots than a" means some key is stored past the wrap."""
import numpy as np

MUL = np.uint64(0x9E3779B97F4A7C15)
LDS_SLOTS = 2048
BLOCK = 1024
FIELD = (1 << 21) - 1
INT64_MIN = -(1 << 63)


# ---------------------------------------------------------------------------------------------------- the key
def quant(v, res):
    """int64 per value: float32 product with float32(1) / float32(res), half away from zero; outside int64 -> INT64_MIN."""
    inv = np.float32(1) / np.float32(res)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.asarray(v, dtype=np.float32) * inv).astype(np.float32)      # the float32 product, rounded once
    t64 = t.astype(np.float64)
    # (|t| >= 2^23 is an integer already; below that t + 0.5 is exact in float64)
    r = np.where(np.abs(t64) < 2.0 ** 23, np.trunc(t64 + np.copysign(0.5, t64)), t64)
    ok = (r >= -2.0 ** 63) & (r < 2.0 ** 63)
    q = np.where(ok, r, 0.0).astype(np.int64)
    return np.where(ok, q, np.int64(INT64_MIN))


def field(q64):
    """The 21-bit field of an axis: low 32 bits as int32, + 2^20, masked."""
    q32 = (np.asarray(q64, dtype=np.int64) & np.int64(0xffffffff)).astype(np.uint32).view(np.int32)
    return ((q32.astype(np.int64) + (1 << 20)) & FIELD).astype(np.uint64)


def key(xyz, res):
    """uint64 key per row of an (n, 3) float32 array."""
    f = field(quant(np.asarray(xyz, dtype=np.float32).reshape(-1, 3), res))
    return f[:, 0] | (f[:, 1] << np.uint64(21)) | (f[:, 2] << np.uint64(42))


def key_of_q(q):
    """Key of integer voxel coordinates (n, 3)."""
    f = field(np.asarray(q, dtype=np.int64).reshape(-1, 3))
    return f[:, 0] | (f[:, 1] << np.uint64(21)) | (f[:, 2] << np.uint64(42))


def hash_(k):
    with np.errstate(over="ignore"):
        return np.asarray(k, dtype=np.uint64) * MUL


def lds_home(k):
    return ((hash_(k) >> np.uint64(40)) & np.uint64(LDS_SLOTS - 1)).astype(np.int64)


def hbm_home(k, cap):
    return ((hash_(k) >> np.uint64(20)) & np.uint64(cap - 1)).astype(np.int64)


def capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


# ---------------------------------------------------------------------------------------------------- points of a cloud
def xyz_of(cloud, step, off):
    """(n, 3) float32 of the triple at `off` of every `step`-byte point."""
    pts = np.asarray(cloud, dtype=np.uint8).reshape(-1, step)
    return np.ascontiguousarray(pts[:, off:off + 12]).view(np.float32).reshape(-1, 3)


def finite(xyz):
    bits = np.ascontiguousarray(xyz, dtype=np.float32).view(np.uint32).reshape(-1, 3)
    return np.all((bits & np.uint32(0x7f800000)) != np.uint32(0x7f800000), axis=1)


def blocks(n):
    """[(lo, hi)) of the 1024-point blocks of a cloud of n points."""
    return [(lo, min(n, lo + BLOCK)) for lo in range(0, n, BLOCK)]


def block_firsts(keys, fin):
    """Per block: the cloud-local indexes of the lowest point per distinct key among its finite points, ascending. These are
    the points that go on to the HBM table."""
    out = []
    for lo, hi in blocks(len(keys)):
        idx = lo + np.flatnonzero(fin[lo:hi])
        _, first = np.unique(keys[idx], return_index=True)
        out.append(idx[np.sort(first)])
    return out


def survivors(cloud, step, off, res):
    """Indexes of the first occurrence per key among the finite points, in order."""
    xyz = xyz_of(cloud, step, off)
    fin = finite(xyz)
    idx = np.flatnonzero(fin)
    _, first = np.unique(key(xyz[idx], res), return_index=True)
    return idx[np.sort(first)]


def survivor_bytes(cloud, step, off, res):
    pts = np.asarray(cloud, dtype=np.uint8).reshape(-1, step)
    return pts[survivors(cloud, step, off, res)].reshape(-1)


# ---------------------------------------------------------------------------------------------------- tables
def occupied(homes, size):
    """The final set of occupied slots (bool [size]) after inserting one distinct key per entry of `homes` with linear
    probing and wrap-around. Independent of the insertion order."""
    occ = np.zeros(size, dtype=bool)
    for h in np.asarray(homes, dtype=np.int64):
        h = int(h)
        while occ[h]:
            h = (h + 1) % size
        occ[h] = True
    return occ


def chain_bound(home, occ):
    """Slots from `home` to the first free slot of the final table: no probe that starts at `home` walks further."""
    size = len(occ)
    d = 0
    while occ[(home + d) % size]:
        d += 1
        assert d < size
    return d


def stored_past_the_wrap(homes, size):
    """True if, for some a, more than a distinct keys home in the last a slots: one of them is stored at slot 0 or behind,
    whatever the order of the inserts."""
    homes = np.asarray(homes, dtype=np.int64)
    per_slot = np.bincount(homes, minlength=size)
    in_last = np.cumsum(per_slot[::-1])                          # in_last[a - 1] = keys homing in the last a slots
    return bool(np.any(in_last > np.arange(1, size + 1)))


def lds_facts(keys):
    """Of the distinct keys of ONE block: (wraps, longest chain bound, occupied)."""
    k = np.unique(np.asarray(keys, dtype=np.uint64))
    homes = lds_home(k)
    occ = occupied(homes, LDS_SLOTS)
    return stored_past_the_wrap(homes, LDS_SLOTS), max(chain_bound(int(h), occ) for h in homes), occ


def hbm_facts(cloud, step, off, res):
    """Of one cloud: (cap, wraps, longest chain bound, occupied, keys that reach the table, inserts per key). A key is
    inserted once per block that holds it (by that block's first point of it)."""
    xyz = xyz_of(cloud, step, off)
    keys, fin = key(xyz, res), finite(xyz)
    cap = capacity(len(keys))
    firsts = block_firsts(keys, fin)
    sent = np.concatenate([keys[f] for f in firsts]) if firsts else np.zeros(0, np.uint64)
    k, inserts = np.unique(sent, return_counts=True)
    if k.size == 0:
        return cap, False, 0, np.zeros(cap, dtype=bool), k, inserts
    homes = hbm_home(k, cap)
    occ = occupied(homes, cap)
    return cap, stored_past_the_wrap(homes, cap), max(chain_bound(int(h), occ) for h in homes), occ, k, inserts


# ---------------------------------------------------------------------------------------------------- gather
def copy_branch(step, src_addr, dst_addr):
    if step % 16 == 0 and (src_addr | dst_addr) % 16 == 0:
        return "uint4"
    if step % 4 == 0 and (src_addr | dst_addr) % 4 == 0:
        return "dword"
    return "byte"


def load_branch(addr):
    """viz_load_f32: one aligned load, or four bytes."""
    return "aligned" if addr % 4 == 0 else "bytes"


def ranks_shifted_stay_inside(keep_counts_per_wave_per_block, total_points):
    """For the `lane <= wave` mutant of the gather prefix: wave w of a block would add its own count to its rank. The
    largest rank any survivor would then take, against the output capacity in points."""
    worst, base = 0, 0
    for waves in keep_counts_per_wave_per_block:
        before = 0
        for c in waves:
            if c:
                worst = max(worst, base + before + c + c - 1)
            before += c
        base += before
    return worst < total_points


# ---------------------------------------------------------------------------------------------------- key picker
class KeyBox:
    """The keys of the integer box [lo, hi)^3 (or [lo[a], hi[a]) per axis) with their homes, and pickers of distinct keys by
    home. The HBM home of a cap-slot table reads hash bits 20 .. 20 + log2(cap) - 1, which depend on key bits 0 .. 33 alone: on x
    and the low 13 bits of y, never on z. A table of 16384 slots needs a box wider than 128 in x and y to fill every home."""

    def __init__(self, lo=-64, hi=64):
        lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
        r = [np.arange(lo[a], hi[a], dtype=np.int64) for a in range(3)]
        q = np.stack(np.meshgrid(*r, indexing="ij"), axis=-1).reshape(-1, 3)
        self.q = q
        self.keys = key_of_q(q)
        self.lds = lds_home(self.keys)
        self._order = np.argsort(self.lds, kind="stable")
        self._start = np.searchsorted(self.lds[self._order], np.arange(LDS_SLOTS + 1))

    def with_lds_home(self, s):
        """Indexes (into q / keys) of every key of the box homing on LDS slot s."""
        return self._order[self._start[s]:self._start[s + 1]]

    def same_lds(self, s, m, cap=None):
        """m keys homing on LDS slot s; with `cap`, their HBM homes pairwise distinct."""
        idx = self.with_lds_home(s)
        if cap is not None:
            _, first = np.unique(hbm_home(self.keys[idx], cap), return_index=True)
            idx = idx[np.sort(first)]
        assert idx.size >= m, (s, m, cap, idx.size)
        return idx[:m]

    def same_hbm(self, cap, slot, m, exclude_lds=()):
        """m keys homing on HBM slot `slot` of a cap-slot table, LDS homes pairwise distinct and none in exclude_lds."""
        idx = np.flatnonzero(hbm_home(self.keys, cap) == slot)
        _, first = np.unique(self.lds[idx], return_index=True)
        idx = idx[np.sort(first)]
        idx = idx[~np.isin(self.lds[idx], np.asarray(list(exclude_lds), dtype=np.int64))]
        assert idx.size >= m, (cap, slot, m, idx.size)
        return idx[:m]

    def same_both(self, cap, m):
        """m keys that share the LDS home AND the HBM home (cap slots): the first such group of the box."""
        both = self.lds * cap + hbm_home(self.keys, cap)
        order = np.argsort(both, kind="stable")
        b = both[order]
        run = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
        length = np.diff(np.concatenate([run, [b.size]]))
        at = np.flatnonzero(length >= m)
        assert at.size, (cap, m)
        return order[run[at[0]]:run[at[0]] + m]



def keys_in_box(lo, hi):
    """The keys of the integer box [lo, hi)^3, with the pickers by home."""
    return KeyBox(lo, hi)
