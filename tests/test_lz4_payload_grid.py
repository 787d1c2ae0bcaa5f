"""The payload grid of the device LZ4 encoder (tests/lz4_payload_grid.py) on the CPU: the raw-byte schemas hand the compressor
the bytes the grid chose, every case reaches the branch it was built for (by the model's trace, Oracle.lz4_trace), the trace
agrees with the model it shares its parser with, and the model's block of every case is valid LZ4 for the system's liblz4.
The device side is tests/test_gpu_lz4_encode_grid.py."""
import collections

import numpy as np
import pytest

import lz4_payload_grid as G
from test_device_lz4 import _chunks, _lz4_decompress

_traces = {}


def traces(oracle, stage2):
    """per case of the parameter set: the trace of every chunk of every cloud, in order (computed once)"""
    if stage2 not in _traces:
        _traces[stage2] = {c.id: [oracle.lz4_trace(p, *G.PARAMS[stage2]) for cloud in c.clouds for p in G.chunk_payloads(c.schema, cloud)]
                           for c in G.grid(stage2)}
    return _traces[stage2]


def _raw_cloud(name):
    step = G.STEPS[name]
    n = 40000 if step < 32 else 33000                            # two chunks; RAW32: 1 MiB and 7424 bytes
    return G.filler(n * step), n


@pytest.mark.parametrize("name", sorted(G.STEPS))
def test_the_payload_of_a_raw_schema_is_the_points(oracle, name):
    data, n = _raw_cloud(name)
    got = _chunks(oracle.encode_stage1(G.schema(name, n), data))
    want = G.chunk_payloads(name, data)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("name", sorted(G.STEPS))
def test_the_payload_of_a_raw_schema_is_the_points_for_the_reference(reflib, name):
    data, n = _raw_cloud(name)
    got = _chunks(reflib.encode_stage1(G.schema(name, n), data))
    want = G.chunk_payloads(name, data)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("stage2", [1, 2])
def test_the_filler_has_no_match(oracle, stage2):
    """every case starts from a sub-range aligned stretch of the filler: no sub-range of it holds a match"""
    P = G.PARAMS[stage2]
    assert G.FILL_STRETCH % P[0] == 0
    t = oracle.lz4_trace(G.fill_bytes(), *P)
    assert len(t.subs) == G.FILL_BYTES // P[0] and len(t.matches) == 0 and not t.subs["full"].any()
    assert t.size == 1 + G.ext_bytes(G.FILL_BYTES) + G.FILL_BYTES


@pytest.mark.parametrize("stage2", [1, 2])
@pytest.mark.parametrize("family", sorted(G.FAMILIES))
def test_every_case_reaches_its_branch_and_its_model_block_is_valid(oracle, family, stage2):
    P = G.PARAMS[stage2]
    T = traces(oracle, stage2)
    n = 0
    for c in G.grid(stage2):
        if c.family != family:
            continue
        n += 1
        c.cond(T[c.id])                                                         # the condition the case was built for
        payloads = [p for cloud in c.clouds for p in G.chunk_payloads(c.schema, cloud)]
        assert len(payloads) == len(T[c.id])
        for p, t in zip(payloads, T[c.id]):
            block = oracle.lz4_model(p, *P)
            assert t.size == block.size, c.id                                   # the layout's size is the model's
            lit = p.size - int(t.subs["last_end"].max())                          # the last sequence: literals only
            assert int(t.subs[-1]["before"]) + int(t.subs[-1]["sub_size"]) + 1 + G.ext_bytes(lit) + lit == block.size, c.id
            assert _lz4_decompress(block, p.size) == p.tobytes(), c.id
    assert n > 0


def _reach(T, P):
    sub = P[0]
    k_img = sub + G.K_IMG_EXTRA
    r = collections.Counter()
    lengths = set()
    for ts in T.values():
        for t in ts:
            span = t.subs["span"].astype(np.int64)
            r["direct"] += int((span > k_img).sum())                                   # lz_emit_direct at any address
            r["below"] += int(((span + 15 <= k_img) & (span + 31 > k_img)).sum())      # the LDS image at any address, by < 16 bytes
            r["address_decides"] += int(((span <= k_img) & (span + 15 > k_img)).sum())
            r["full"] += int(t.subs["full"].sum())
            r["steps_of_16"] += int((t.steps[:, 1] == 16).sum())
            r["steps_past_their_end"] += int((t.steps[:, 2] > 64).sum())
            r["wide_chunks"] += int(len(t.subs) > 64)
            r["chunks"] += 1
            r["sub_ranges"] += len(t.subs)
            lengths |= set(int(x) for x in t.matches[:, 1])
    return r, lengths


@pytest.mark.parametrize("stage2", [1, 2])
def test_what_the_grid_reaches(oracle, stage2):
    """conditions on the inputs, from the model's trace alone (not measurements)"""
    P = G.PARAMS[stage2]
    r, lengths = _reach(traces(oracle, stage2), P)
    per_family = collections.Counter(c.family for c in G.grid(stage2))
    payload = sum(cloud.size for c in G.grid(stage2) for cloud in c.clouds)
    print(f"lz4 payload grid, parameters {P}: {len(G.grid(stage2))} cases (" + ", ".join(f"{f}: {per_family[f]}" for f in sorted(per_family)) +
          f"), {payload} payload bytes; " + ", ".join(f"{k} {v}" for k, v in sorted(r.items())) + f", {len(lengths)} match lengths")
    assert sorted(per_family) == sorted(G.FAMILIES)
    assert r["direct"] >= 17 and r["below"] >= 6 and r["address_decides"] >= 15
    assert len(lengths) >= 24 and set(G.MATCH_LENGTHS + [P[0] - 200]) <= lengths
    assert r["full"] >= 1 and r["steps_of_16"] >= 1 and r["steps_past_their_end"] >= 3 and r["wide_chunks"] >= 1
    assert payload < 64 << 20
    keys = set(G.batches(stage2))
    assert keys == set(G.BATCH_KEYS)


def test_trace_and_model_agree_beyond_the_grid(oracle):
    """the trace shares lz4m_parse with the model: sizes and sequence bytes agree on the payload kinds of test_device_lz4 too"""
    from test_device_lz4 import _payload_kinds
    for n in (0, 1, 12, 13, 70, 4096, 8193, 20000):
        for kind, payload in _payload_kinds(np.random.RandomState(n), n):
            for P in ((8192, 11, 1024), (4096, 10, 512), (64, 4, 3), (100, 6, 1 << 20)):
                t = oracle.lz4_trace(payload, *P)
                assert t.size == oracle.lz4_model(payload, *P).size, (n, kind, P)
                anchor = 0
                for k, r in enumerate(t.subs):                                     # anchors chain, matches stay inside their sub-range
                    assert int(r["anchor_in"]) == anchor
                    m = t.sub_matches(k)
                    if len(m):
                        assert int(m[0][0]) >= int(r["s"]) + 64 and int(m[-1][0] + m[-1][1]) <= int(r["e"])
                        assert all(int(x[2]) <= int(x[0]) - int(r["s"]) for x in m)
                        anchor = int(r["last_end"])
                    assert int(r["count"]) == sum(int(s[1]) for s in t.sub_steps(k))
