"""The near-tie grid of tests/probe_tie_cases.py on the CPU: every row is what it says, the grid covers what it claims (computed from
the rows, not assumed), the model's verdict on every row is the oracle's, the oracle's bytes are the compiled reference's, and -- the
point of the grid -- a one-byte error in any of the four section sizes changes the verdict on some row of every width and length
class. No GPU."""
import itertools

import numpy as np
import pytest

import cases
import mode_model as M
import probe_tie_cases as P

F = cases.F
PAIR, TERM, TINY, SUMS = (P.rows(f) for f in ("pair", "term", "tiny", "sums"))
ALL_CELLS = {(a, b, d) for (a, b), d in itertools.product(P.PAIRS, P.DIFFS)}
CLASSES = ("mid", "full", "beyond")


def test_every_condition_holds_and_names_are_unique():
    assert len({r[0] for r in P.ROWS}) == len(P.ROWS)
    for name, family, ftype, values, cond in P.ROWS:
        assert values.dtype == P.NP[ftype] and values.ndim == 1 and values.size, name
        assert cond(values), name
        assert family in ("pair", "term", "tiny", "sums"), name


def test_pair_coverage():
    """pair x diff x width x length class, from the rows' own sizes: all 18 cells in every class at every width (so the list of
    unreached cells is empty), both types of every width in every class."""
    table = {}
    for name, _f, ftype, values, _c in PAIR:
        cell = P.pair_cell(values[:P.PROBE])
        assert cell is not None, name
        table.setdefault((P.WIDTH_OF[ftype], P.length_class(values)), {}).setdefault(cell, set()).add(ftype)
    for w in P.WIDTHS:
        for cls in CLASSES:
            assert set(table[(w, cls)]) == ALL_CELLS, (w, cls, ALL_CELLS - set(table[(w, cls)]))
            assert {t for ts in table[(w, cls)].values() for t in ts} == set(P.TYPES_OF[w]), (w, cls)
    assert not [u for u in P.UNREACHED if u[0] == "pair"]
    for name, _f, _t, values, _c in PAIR:
        if P.length_class(values) == "mid":
            assert 1025 < values.size < 4096 and values.size % 16


EVERY_WIDTH = ["value_run_127_128_" + x for x in ("at_256", "at_1024", "at_end", "behind_4096")] + \
    ["delta_run_127_128_" + x for x in ("at_256", "at_1024", "at_end", "behind_4096")] + \
    ["palette_u_%d" % u for k in (0, 1, 2, 4, 8, 11) for u in (1 << k, (1 << k) + 1)] + \
    ["all_ones_value", "all_ones_value_signed", "index_bytes_mod8_0", "index_bytes_mod8_1", "run_over_two_waves", "first_value_token"]
STEPS_OF = {2: 2, 4: 4, 8: 9}   # varint64_len steps a delta of the width reaches: 2^(7k - 1) <= 2^(8w) - 1


def test_term_coverage():
    want = {t: set(P.WIDTHS) for t in EVERY_WIDTH}
    for w, steps in STEPS_OF.items():
        for k in range(1, steps + 1):
            assert (1 << (7 * k - 1)) < (1 << (8 * w)) and (k == steps or k < 9)
            for way in ("rising", "falling"):
                want.setdefault(f"varint_step_{k}_{way}", set()).add(w)
    want["int64_min_delta"] = want["int64_wrap_around_delta"] = {8}
    assert {t: set(ws) for t, (_m, ws) in P.TERMS.items()} == want
    names = {n for _m, ws in P.TERMS.values() for tr in ws.values() for n in tr} | {n for pair in P.SAME_RAW for n in pair}
    assert names == {r[0] for r in TERM}
    (u, i), = P.SAME_RAW
    assert P.BY_NAME[u][3].tobytes() == P.BY_NAME[i][3].tobytes() and (P.BY_NAME[u][2], P.BY_NAME[i][2]) == (F.UINT16, F.INT16)
    assert M.select(P.window_sizes(P.BY_NAME[u][3])) != M.select(P.window_sizes(P.BY_NAME[i][3]))


def test_tiny_and_sums_coverage():
    per_type = {}
    for _n, _f, ftype, values, _c in TINY:
        per_type.setdefault(ftype, set()).add(tuple(values.tolist()))
    for ftype in (t for w in P.WIDTHS for t in P.TYPES_OF[w]):
        k = 6 if ftype in P.SIGNED else 5                     # (an unsigned type's maximum is its all-ones value)
        assert len(per_type[ftype]) == k + k ** 2 + k ** 3 + k ** 4
        ones = -1 if ftype in P.SIGNED else int(np.iinfo(P.NP[ftype]).max)
        assert {x for col in per_type[ftype] for x in col} == {0, 1, 63, 64, int(np.iinfo(P.NP[ftype]).max), ones}
    # DeltaVarint (1 + n small tokens) wins most of these outright: about one column in nine has its two smallest sizes within a byte
    # of each other, fewer the wider the type (Palette and Rle pay for every value they hold)
    near = {}
    for r in TINY:
        low = sorted(P.window_sizes(r[3]))
        near[r[2]] = near.get(r[2], 0) + (low[1] - low[0] <= 1)
    assert sum(near.values()) >= 800, near
    cells = {w: set() for w in P.WIDTHS}
    for name, _f, ftype, values, _c in SUMS:
        t = P.whole_sizes(values)
        a, b = sorted(sorted(range(4), key=lambda m: (t[m], m))[:2])
        cells[P.WIDTH_OF[ftype]].add((a, b, t[a] - t[b]))
        assert values.size == P.CHUNK + 300
    assert all(c == ALL_CELLS for c in cells.values()) and not P.UNREACHED


def _flips(sizes, m, e):
    moved = list(sizes)
    moved[m] += e
    return M.select(moved) != M.select(sizes)


def test_sensitivity_a_one_byte_error_in_any_size_changes_a_verdict():
    """For each mode m and each e in {-1, +1}: rows on which select() changes when sizes[m] alone moves by e -- at least one per
    width and length class. A kernel whose size m is off by e commits another mode than the model on those rows."""
    count = {}
    for _n, _f, ftype, values, _c in PAIR:
        s = P.window_sizes(values)
        for m in range(4):
            for e in (-1, 1):
                if _flips(s, m, e):
                    key = (m, e, P.WIDTH_OF[ftype], P.length_class(values))
                    count[key] = count.get(key, 0) + 1
    for key in itertools.product(range(4), (-1, 1), P.WIDTHS, CLASSES):
        assert count.get(key, 0) >= 1, key


def test_sensitivity_every_term_triple_is_separated_by_its_own_term():
    """Moving the term's size by one on the tie row gives the neighbour's verdict, for both neighbours, and one of them differs from
    the tie's: the triple cannot pass with the term off by one in either direction."""
    for term, (m, widths) in P.TERMS.items():
        for w, (tie, minus, plus) in widths.items():
            s = P.window_sizes(P.BY_NAME[tie][3])
            verdicts = []
            for name, e in ((minus, -1), (plus, 1)):
                moved = list(s)
                moved[m] += e
                got = M.select(P.window_sizes(P.BY_NAME[name][3]))
                assert M.select(moved) == got, (term, w, name)
                verdicts.append(got)
            assert set(verdicts) != {M.select(s)}, (term, w)
            assert _flips(s, m, -1) or _flips(s, m, 1)


def _layout(row):
    return cases.int_only(row[3], row[2])


def test_model_against_the_oracle_on_every_row(oracle):
    for row in P.ROWS:
        info, data = _layout(row)
        _stream, probed = oracle.encode_stage1(info, data, return_modes=True)
        assert probed.tolist() == [M.select(P.window_sizes(row[3]))], row[0]
    for row in SUMS + [r for r in PAIR if P.length_class(r[3]) == "beyond"]:
        info, data = _layout(row)
        rep = M.sweep(info, data, [row[3].size])[0, 0]
        assert rep["bytes"].tolist() == P.whole_sizes(row[3]) and rep["best_mode"] == M.select(P.whole_sizes(row[3])), row[0]
        # the sizes are what forcing each mode does to the oracle's stream
        sizes = [oracle.encode_stage1_continued(info, data, np.array([m], np.uint8)).size for m in range(4)]
        assert len({z - int(b) for z, b in zip(sizes, rep["bytes"])}) == 1, row[0]


def test_oracle_against_the_compiled_reference_on_pair_and_term_rows(oracle, reflib):
    for row in PAIR + TERM:
        info, data = _layout(row)
        assert reflib.encode_stage1(info, data).tobytes() == oracle.encode_stage1(info, data).tobytes(), row[0]
