"""Constructed integer columns for the V5 section WRITERS, shared by tests/test_section_cases.py (model against oracle and
reference, no GPU) and tests/test_gpu_sections.py (device against model, every mode forced). tests/mode_cases.py aims at the
edges of the mode sweep, which only measures; these aim at the edges of the kernels that write:

  thread    section_runs_body (stage1_sections.h) gives 32 values to a thread and closes a thread's last run with a suffix-min
            over the later threads: run heads on value 32k - 1, 32k, 32k + 1
  tile      section_runs (stage1_kernels.hip) walks tiles of 1024 values and carries the open run: heads on 1024k - 1, 1024k,
            1024k + 1, tiles without any head (runs of 2049 and longer)
  quarter   section_delta32_body works in quarters of 8192 values and keeps the partial 16-byte unit for the next one
  residue   the section size after each quarter is 0, 1 and 15 mod 16; total sizes of 16, 17, 65535 and 65537 bytes
  token     varints of every length the width can reach (3, 5 and 10 bytes), LEB128 run lengths of 1, 2 and 3 bytes
  capacity  3072 / 3073 distinct values (kS2PalCapacity), 6144 / 6145 (kPalCapacity), 32768, and the hashes that split them

A case is (name, values before the cast to the field type, check, edges, outcome). check(v) takes the column as the model sees
it (int64) and is False when the column does not have the property it was built for: a case cannot pass for another reason.
edges names what the case reaches, asserted as a coverage table by tests/test_section_cases.py. outcome says what a forced
Palette must give on the device: MODEL (the model's bytes) or REFUSED (the call fails with ST_PALETTE_FULL and writes nothing
outside its output)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import cases
import mode_cases as MC
import mode_model as M
import section_model as S

F = cases.F
CHUNK = M.CHUNK
TYPES = MC.TYPES
_NP = MC._NP
MODEL, REFUSED = "model", "refused"
EDGES = ("thread", "tile", "quarter", "residue", "token", "capacity")
SECTION_STRIDE = 409600                 # kSectionStride: the room one section has in a chunk's slot
S2_PAL_CAPACITY, PAL_CAPACITY = 3072, 6144  # kS2PalCapacity (k_section_palette, Pal32), kPalCapacity (section_palette)
PAL_FIRST_PARTS, PAL_MAX_PARTS = 8, 4096    # section_palette: partitions of the second attempt, of the last
PAL32_PARTS = (32, 128, 512, 2048, 8192)    # pal32_slow_first

Case = namedtuple("Case", "name values check edges outcome")
INT64_MIN_DELTA = "delta_of_int64_min"
UNDECODABLE = {(INT64_MIN_DELTA, 0), (INT64_MIN_DELTA, 3)}  # (case, mode) streams every decoder refuses, the reference's first

LENGTHS = [1, 2, 31, 32, 33, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769]
RUN_LENGTHS = [[16384, 1, 2, 31, 32, 33, 63, 64], [16383, 65, 127, 128, 1023, 1024, 1025, 2049]]  # chunk 0, chunk 1


def bits_of(ftype):
    return 8 * np.dtype(_NP[ftype]).itemsize


def limits(ftype):
    i = np.iinfo(_NP[ftype])
    return int(i.min), int(i.max)


def sec_part(raw, parts):
    """section_palette's partition of the raw (zero-extended) values: (hash_u64 >> 20) % parts, hash_u64 the low half of mix."""
    return ((MC.mix(raw) & np.uint64(0xffffffff)) >> np.uint64(20)) % np.uint64(parts)


def sec_parts_needed(raw):
    """The partition count section_palette ends with: 1, else 8 doubled while a partition overflows; 0 past PAL_MAX_PARTS."""
    keys = np.unique(raw)
    if keys.size <= PAL_CAPACITY:
        return 1
    parts = PAL_FIRST_PARTS
    while parts <= PAL_MAX_PARTS:
        if np.bincount(sec_part(keys, parts).astype(np.int64), minlength=parts).max() <= PAL_CAPACITY:
            return parts
        parts *= 2
    return 0


def pal32_hash(v):
    """The mixer of pal32_part for 32-bit keys; the partition of P is its top log2(P) bits."""
    h = (v.astype(np.uint64) * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    return (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)


def pal32_unhash(h):
    """The inverse of pal32_hash (both multipliers are odd, the shift-xor is its own inverse after two more terms)."""
    h = (h.astype(np.uint64) * np.uint64(pow(0xc2b2ae35, -1, 1 << 32))) & np.uint64(0xffffffff)
    h = h ^ (h >> np.uint64(15)) ^ (h >> np.uint64(30))
    return (h * np.uint64(pow(0x85ebca6b, -1, 1 << 32))) & np.uint64(0xffffffff)


def pal32_parts_needed(raw):
    """The partition count pal32_slow_first ends with for 32-bit keys (0: none of PAL32_PARTS fits), 1 if it is never entered."""
    keys = np.unique(raw)
    if keys.size <= S2_PAL_CAPACITY:
        return 1
    for parts in PAL32_PARTS:
        if np.bincount(((pal32_hash(keys) * np.uint64(parts)) >> np.uint64(32)).astype(np.int64), minlength=parts).max() <= S2_PAL_CAPACITY:
            return parts
    return 0


def _heads(v, delta):
    return S.run_heads(S.deltas(v).view(np.uint64) if delta else v.view(np.uint64))


def _runs_at(v, delta):
    """(start, length) of every run of one section."""
    h = np.flatnonzero(_heads(v, delta))
    return h, np.diff(np.append(h, v.size))


def _has_runs(v, delta, lens, mod, at):
    """Every length of `lens` is the length of a run of the section whose head lies on a value = at (mod `mod`)."""
    start, length = _runs_at(v, delta)
    return all(((length == L) & (start % mod == at % mod)).any() for L in lens)


def _varint_lens(v):
    return M._varint64_len(S.deltas(v))


def _placed_runs(lens, mod, at, delta, base):
    """One chunk: runs of the given lengths, each head on the next value = at (mod `mod`), single values in between and
    behind, 32768 values in all. delta: the runs are runs of equal first differences (the values all differ)."""
    keys, pos, k = [], 0, 0

    def filler(count):
        nonlocal pos
        for _ in range(count):
            keys.append(7 if (pos & 1) else -7) if delta else keys.append(40000 + (pos & 1))
            pos += 1
    level = 0
    for L in lens:
        if delta and pos == 0 and at % mod == 0:
            filler(mod)  # (a section's first difference is taken against 0: it belongs to no run of the ramp)
        filler((at - pos) % mod)
        if delta:
            mag = 1 if L > 4096 else 1 + (k & 1)
            key = -mag if level > 0 else mag
            if keys and keys[-1] == key:
                key = -key
            level += key * L
        else:
            key = 11 + 37 * k
        keys.extend([key] * L)
        pos += L
        k += 1
    assert pos <= CHUNK, (pos, lens, mod, at)
    filler(CHUNK - pos)
    keys = np.array(keys, dtype=np.int64)
    return base + np.cumsum(keys) if delta else keys


def _family_a(ftype, add):
    for n in LENGTHS:
        i = np.arange(n)
        add(f"len_{n}_ramp", np.where(i < n // 2, i, n // 2 + 3 * (i - n // 2)) % 30000, lambda v, n=n: v.size == n, ())
        add(f"len_{n}_runs_of_3", (i // 3) * 5 % 30000,
            lambda v, n=n: v.size == n and (_runs_at(v[:CHUNK], False)[1][:-1] == 3).all(), ())


def _family_b(ftype, add):
    lo, _hi = limits(ftype)
    base = 0 if lo < 0 else 32768
    for mod, edge in ((32, "thread"), (1024, "tile")):
        for at in (-1, 0, 1):
            for delta in (False, True):
                v = np.concatenate([_placed_runs(RUN_LENGTHS[c], mod, at, delta, base) for c in (0, 1)])
                add(f"runs_{'delta' if delta else 'value'}_{edge}_{'m1' if at < 0 else 'p%d' % at}", v,
                    lambda v, mod=mod, at=at, delta=delta: all(_has_runs(v[c * CHUNK:(c + 1) * CHUNK], delta, RUN_LENGTHS[c], mod, at)
                                                                for c in (0, 1)),
                    (edge, "tile") if edge == "thread" else (edge,))  # (2049 values hold a whole tile wherever they start)
    rs = np.random.RandomState(77)
    lo, hi = limits(ftype)
    big = np.array([rs.randint(lo // 2, hi // 2) for _ in range(200)], dtype=np.int64)  # (python ints: the range of any type)
    add("runs_of_5_of_scattered_values", np.repeat(big, 5),
        lambda v, bpv=bits_of(ftype) // 8: M.select(M.section_sizes(v, bpv)) == 2, ())        # the reference's probe commits Rle
    add("one_run_32768_of_zero", np.zeros(CHUNK, dtype=np.int64),
        lambda v: _runs_at(v, False)[1].tolist() == [CHUNK] and _runs_at(v, True)[1].tolist() == [CHUNK], ("tile", "token"))
    add("one_run_32768_of_five", np.full(CHUNK, 5),
        lambda v: _runs_at(v, False)[1].tolist() == [CHUNK] and _runs_at(v, True)[1].tolist() == [1, CHUNK - 1], ("tile", "token"))


def max_delta_token_bytes(bpv):
    """Bytes of the longest varint a difference of two values of that many bytes can take."""
    return {2: 3, 4: 5, 8: 10}[bpv]


def max_delta_token(ftype):
    return max_delta_token_bytes(bits_of(ftype) // 8)


def _family_c(ftype, add):
    lo, hi = limits(ftype)
    bpv = bits_of(ftype) // 8
    far = (1 << 62) if bpv == 8 else hi  # (UINT64: 0 <-> 2^63 would be the same difference both ways, INT64_MIN)
    near = 0 if bpv == 8 else lo
    v = np.where(np.arange(CHUNK) % 2 == 0, far, near)
    if bpv == 8:
        v = v.astype(np.uint64 if ftype == F.UINT64 else np.int64)

    def check(v, bpv=bpv, tok=max_delta_token(ftype)):
        sizes = M.section_sizes(v, bpv)
        return (sizes[2] == 5 + CHUNK * (bpv + 1) and sizes[3] == 5 + CHUNK * (tok + 1) and sizes[0] == 1 + CHUNK * tok
                and max(sizes) < SECTION_STRIDE)
    add("every_value_its_own_run_longest_tokens", v, check, ("token",))


def _delta_for(u):
    """The difference whose zig-zag(+1) word is u."""
    z = u - 1
    return (z >> 1) ^ -(z & 1)


def _family_d(ftype, add):
    lo, hi = limits(ftype)
    bits = bits_of(ftype)
    span = hi - lo
    words = []
    for k in range(1, max_delta_token(ftype) + 1):
        words += [1 << (7 * k - 1), (1 << (7 * k)) - 1, 1 << (7 * k)]  # exactly 7k bits (smallest, largest), 7k + 1 bits
    words = [u for u in words if u < (1 << 64) and abs(_delta_for(u)) <= span]
    seq = []
    for u in words:
        d = _delta_for(u)
        seq += [lo, lo + d] if d > 0 else [lo - d, lo]
    # min to max and back: 0 -> 0xFFFFFFFF for UINT32. (64 bits: INT64_MIN - 0 would be the difference of INT64_MIN, which has
    # a case of its own below, so no 0 follows the minimum and -1 stands in front of it)
    seq = ([-1] if ftype == F.INT64 else []) + seq + ([lo, hi, lo, hi] if bits == 64 else [lo, hi, lo, 0, hi])
    if bits == 16:
        seq += [0, 0x8000 if lo == 0 else -0x8000, 0]            # the raw bits 0x8000 are +32768 in one type, -32768 in the other
    dt = np.uint64 if ftype == F.UINT64 else np.int64
    v = np.array(seq, dtype=dt)

    def check(v, words=words):
        got = set(S.zigzag1(S.deltas(v)).tolist())
        return set(words) <= got and set(_varint_lens(v).tolist()) >= set(range(1, max_delta_token(ftype) + 1)) and 0 not in got
    add("token_lengths", v, check, ("token",))
    if bits == 64:
        # a difference of INT64_MIN: zig-zag + 1 wraps to 0 and the token is the one byte 00. The reference writes it and its
        # own decoder then takes it for the NaN marker and refuses the stream (DeltaVarint and DeltaRle; UNDECODABLE below)
        add(INT64_MIN_DELTA, np.array([3, 0, 1 << 63 if lo == 0 else -(1 << 63), 0, 5, 5], dtype=dt),
            lambda v: (S.zigzag1(S.deltas(v)) == 0).sum() == 2 and (_varint_lens(v)[S.zigzag1(S.deltas(v)) == 0] == 1).all(), ())
    # the longest token on the last value of a thread, of a quarter and of the chunk, and on the first value of chunk 1,
    # whose difference is taken against 0 and not against chunk 0's last value
    far = (1 << 62) if bits == 64 else (hi if lo == 0 else lo)
    spikes = [31, 8191, CHUNK - 1, CHUNK]
    v = np.zeros(CHUNK + 40, dtype=dt)
    v[spikes] = far

    def check_edges(v, spikes=spikes, tok=max_delta_token(ftype)):
        l0, l1 = _varint_lens(v[:CHUNK]), _varint_lens(v[CHUNK:])
        return all(l0[p] == tok for p in spikes[:3]) and l1[0] == tok and v[CHUNK] == v[CHUNK - 1]
    add("longest_token_on_thread_quarter_chunk_edges", v, check_edges, ("token", "quarter"))  # (check_edges holds the places)


def _toggles(n, positions):
    """0 / 100 values that change at the given positions: each change is one 2-byte token, everything else one byte."""
    flip = np.zeros(n, dtype=np.int64)
    flip[positions] = 1
    return (np.cumsum(flip) % 2) * 100


def _family_e(ftype, add):
    for residue in (0, 1, 15):
        extra = [(residue - 1) % 16, 16, 32, 16]                # 2-byte tokens per quarter: the residue holds after each
        pos = np.concatenate([8192 * q + 100 + 37 * np.arange(e) for q, e in enumerate(extra)]).astype(np.int64)
        add(f"size_{residue}_mod_16_after_every_quarter", _toggles(CHUNK, pos),
            lambda v, r=residue: [(1 + int(_varint_lens(v)[:8192 * (q + 1)].sum())) % 16 for q in range(4)] == [r] * 4,
            ("quarter", "residue"))
    for size, n, two in ((16, 15, False), (17, 16, False), (65535, CHUNK - 1, True), (65537, CHUNK, True)):
        v = _toggles(n, np.arange(n)) if two else np.zeros(n, dtype=np.int64)
        add(f"delta_varint_section_of_{size}_bytes", v, lambda v, size=size: 1 + int(_varint_lens(v).sum()) == size,
            ("residue",))


def _spread(ftype):
    return {16: 1, 32: (1 << 31) // 40000, 64: 1 << 40}[bits_of(ftype)]


def _family_f(ftype, add, rs):
    bits = bits_of(ftype)
    spread = _spread(ftype)
    for u in (1, 2, 3, 256, 257, S2_PAL_CAPACITY, S2_PAL_CAPACITY + 1, PAL_CAPACITY, PAL_CAPACITY + 1, CHUNK):
        n = CHUNK if u == CHUNK else max(1000, u + 300)
        v = (rs.permutation(u)[np.arange(n) % u] + 1) * spread + 5
        add(f"unique_{u}", v, lambda v, u=u: np.unique(v).size == u and v.size <= CHUNK, ("capacity",) if u >= S2_PAL_CAPACITY else ())
    # a value seen for the first time on the last value of chunk 0 (and nowhere in chunk 1)
    v = np.arange(CHUNK + 10) % 7
    v[CHUNK - 1] = 1000
    add("first_occurrence_on_the_last_value_of_a_chunk", v,
        lambda v: np.flatnonzero(v[:CHUNK] == 1000).tolist() == [CHUNK - 1] and not (v[CHUNK:] == 1000).any(), ())
    if bits == 64:
        some = rs.randint(1, 1 << 62, 40, dtype=np.int64)
        body = some[rs.randint(0, 40, 3000)]
        ones = np.int64(-1)
        for where, v in (("first", np.concatenate([[ones], body])), ("last", np.concatenate([body, [ones]])), ("absent", body)):
            v = v.view(np.uint64) if ftype == F.UINT64 else v
            add(f"all_ones_key_{where}", v,
                lambda v, where=where: {"first": v[0] == -1 and (v[1:] != -1).all(), "last": v[-1] == -1 and (v[:-1] != -1).all(),
                                        "absent": (v != -1).all()}[where], ())
        add("upper_half_only", ((rs.permutation(4000)[np.arange(9000) % 4000].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | np.uint64(7),
            lambda v: np.unique(v).size == 4000 and np.unique(v.view(np.uint64) & np.uint64(0xffffffff)).size == 1, ("capacity",))


def _behind_a_quiet_probe(keys, rs):
    """The probe window (4096 values) holds four of the keys, then every key once, then 300 repeats."""
    keys = np.asarray(keys, dtype=np.uint64)
    return np.concatenate([keys[np.arange(M.PROBE) % 4], keys, keys[rs.randint(0, keys.size, 300)]])


def _quiet(v):
    return np.unique(v[:M.PROBE]).size <= 4


def _family_g(ftype, add, rs):
    bits = bits_of(ftype)
    raw = lambda v: S.raw_of(v, bits // 8)
    # keys by section_palette's partition class of 8
    if bits == 64:
        words = np.unique(rs.randint(0, 1 << 62, 90000, dtype=np.int64).astype(np.uint64))
        keys = MC.unmix(rs.permutation(words))
    elif bits == 32:
        keys = rs.permutation(np.unique(rs.randint(0, 1 << 32, 200000, dtype=np.int64).astype(np.uint64)))
    else:
        keys = rs.permutation(1 << 16).astype(np.uint64)
    cls = sec_part(keys, 8)
    one = keys[cls == 0][:7000]
    add("palette_7000_keys_in_one_partition_of_8", _behind_a_quiet_probe(one, rs),
        lambda v: (_quiet(v) and np.unique(v).size == 7000 and (sec_part(np.unique(raw(v)), 8) == 0).all()
                   and sec_parts_needed(raw(v)) == 16), ("capacity",))
    two = np.concatenate([keys[cls == 0][:6100], keys[cls == 1][:6100]])
    add("palette_6100_keys_in_each_of_two_partitions_of_8", _behind_a_quiet_probe(rs.permutation(two), rs),
        lambda v: (_quiet(v) and np.bincount(sec_part(np.unique(raw(v)), 8).astype(np.int64), minlength=8).tolist() == [6100, 6100] + [0] * 6
                   and sec_parts_needed(raw(v)) == 8), ("capacity",))
    if bits == 64:
        # the twelve bits of the partition index all zero: no partition count separates these keys
        words = (np.unique(rs.randint(0, 1 << 30, 9000, dtype=np.int64)).astype(np.uint64)[:PAL_CAPACITY + 56] << np.uint64(32)) | \
            rs.randint(0, 1 << 20, PAL_CAPACITY + 56, dtype=np.int64).astype(np.uint64)
        add("palette_6200_keys_no_partition_count_separates", _behind_a_quiet_probe(MC.unmix(rs.permutation(words)), rs),
            lambda v: (_quiet(v) and np.unique(v).size == PAL_CAPACITY + 56 and (sec_part(np.unique(raw(v)), PAL_MAX_PARTS) == 0).all()
                       and sec_parts_needed(raw(v)) == 0), ("capacity",), REFUSED)
    if bits == 32:
        for count, top, parts in ((3100, 5, 128), (3073, 5, 128), (3100, 7, 512)):
            # the top `top` bits of pal32_part's hash agree, the two bits below them take every value evenly
            low = np.unique(rs.randint(0, 1 << (30 - top), 2 * count, dtype=np.int64))[:count].astype(np.uint64)
            h = (np.uint64(5) << np.uint64(32 - top)) | ((np.arange(count, dtype=np.uint64) % np.uint64(4)) << np.uint64(30 - top)) | low
            add(f"pal32_{count}_keys_agree_in_the_top_{top}_hash_bits", _behind_a_quiet_probe(pal32_unhash(rs.permutation(h)), rs),
                lambda v, count=count, parts=parts: _quiet(v) and np.unique(v).size == count and pal32_parts_needed(raw(v)) == parts,
                ("capacity",))


def grid(ftype):
    """The cases of one field type."""
    rs = np.random.RandomState(313 + int(ftype))
    out = []

    def add(name, v, check, edges, outcome=MODEL):
        assert set(edges) <= set(EDGES)
        out.append(Case(name, np.asarray(v), check, tuple(edges), outcome))
    _family_a(ftype, add)
    _family_b(ftype, add)
    _family_c(ftype, add)
    _family_d(ftype, add)
    _family_e(ftype, add)
    _family_f(ftype, add, rs)
    _family_g(ftype, add, rs)
    return out


_GRIDS = {}


def grid_of(ftype):
    if ftype not in _GRIDS:
        _GRIDS[ftype] = grid(ftype)
    return _GRIDS[ftype]


def layout(case, ftype, odd):
    """(info, data) of the case as a cloud: the field alone at offset 0, or at offset 1 behind a UINT8 (mode_cases.layout)."""
    return MC.layout(case.values, ftype, odd)


def column_of(case, ftype):
    """The case's values as the model sees them (ToInt64<T> of the stored bits)."""
    info, data = layout(case, ftype, False)
    return M.column(info, data, M.adaptive_fields(info)[0])[0]


def pal32_refused_column():
    """(values, check) of a 32-bit column that pal32_slow_first cannot partition: 3100 keys whose pal32_part hash agrees in its top
    13 bits, so that the last count tried (8192 partitions) still holds them all. Kept out of the grid: under section_palette's hash
    (W2, W3) the same column is legal, so it has no one outcome."""
    rs = np.random.RandomState(8192)
    low = np.unique(rs.randint(0, 1 << 19, 8000, dtype=np.int64))[:3100].astype(np.uint64)
    keys = pal32_unhash(rs.permutation((np.uint64(0x155) << np.uint64(19)) | low))
    return _behind_a_quiet_probe(keys, rs), lambda v: (_quiet(v) and np.unique(v).size == 3100 and pal32_parts_needed(S.raw_of(v, 4)) == 0
                                                       and sec_parts_needed(S.raw_of(v, 4)) == 1)


# ---- which test of tests/test_gpu_sections.py sends which cases to which writer ------------------------------------------------
# tests/test_gpu_sections.py takes WIDE_CASES and STALE_CASES from here, and tests/test_section_cases.py asserts that every route
# below names a test that exists and selects at least one case at every width it is for: a route cannot be dropped on one side only.

WIDE_CASES = ("runs_value_tile_m1", "runs_delta_tile_p0", "every_value_its_own_run_longest_tokens", "size_15_mod_16_after_every_quarter",
              "unique_6145", "palette_7000_keys_in_one_partition_of_8", "palette_6100_keys_in_each_of_two_partitions_of_8", "len_1025_ramp")
STALE_CASES = ("runs_value_thread_m1", "runs_value_tile_p0", "runs_delta_thread_p0", "runs_delta_tile_m1", "one_run_32768_of_five",
               "every_value_its_own_run_longest_tokens", "token_lengths", "size_0_mod_16_after_every_quarter", "unique_3073", "unique_6145",
               "palette_7000_keys_in_one_partition_of_8")
FRAMED_TEST, DEVICE_TEST, TABLE_TEST = ("test_every_case_under_every_forced_mode_framed_to_host", "test_framed_to_a_device_buffer_at_every_residue",
                                        "test_chunk_table_call_then_framing")
WIDE_TEST, STALE_TEST = "test_wide_points_every_mode", "test_general_kernel_behind_a_stale_hint"
_ANY = lambda name, u: True
_WIDE = lambda name, u: name in WIDE_CASES
_STALE = lambda name, u: name in STALE_CASES
_SMALL = lambda name, u: u <= S2_PAL_CAPACITY
_LARGE = lambda name, u: u > S2_PAL_CAPACITY
# (writer, mode) -> [(test, widths in bits, selects(case name, most distinct values in one chunk))]
ROUTES = {}
for _m in (0, 2, 3):
    ROUTES[("W1", _m)] = [(FRAMED_TEST, (16, 32), _ANY), (DEVICE_TEST, (16, 32), _ANY), (TABLE_TEST, (16, 32), _ANY)]
    ROUTES[("W2", _m)] = [(FRAMED_TEST, (64,), _ANY), (DEVICE_TEST, (64,), _ANY), (STALE_TEST, (16, 32), _STALE)]
ROUTES[("W2", 1)] = [(FRAMED_TEST, (64,), _LARGE), (TABLE_TEST, (64,), _LARGE), (STALE_TEST, (16, 32), _STALE)]
for _m in (0, 1, 2, 3):
    ROUTES[("W3", _m)] = [(WIDE_TEST, (16, 32, 64), _WIDE)]
ROUTES[("W4", 1)] = [(FRAMED_TEST, (64,), _SMALL), (TABLE_TEST, (64,), _SMALL)]
ROUTES[("W5", 1)] = [(FRAMED_TEST, (16, 32), _ANY), (DEVICE_TEST, (16, 32), _ANY), (TABLE_TEST, (16, 32), _ANY)]
