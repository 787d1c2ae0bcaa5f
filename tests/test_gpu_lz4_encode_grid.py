"""The payload grid of tests/lz4_payload_grid.py through the device LZ4 encoder (cloudini_amd/csrc/lz4_kernels.hip).

Per family, raw-byte schema and parameter set the cases go into one encode_host call as a ragged batch, once in file order and
once reversed (another source and destination alignment for every chunk). For every chunk: the plain stage-1 stream of the
same codec is the oracle's (so the payload is the bytes the grid chose), the block is Oracle.lz4_model's byte for byte and in
size, the system's liblz4 decodes it to the payload, chunk_sizes and the stream offsets are consistent, and decode_lz4_host
returns the points. Family i (the span threshold between the LDS image and lz_emit_direct, where the output ADDRESS mod 16
decides) is also written through encode_device at 0, 1, 7 and 15 bytes from a 256-byte aligned buffer.
That every case reaches the branch it was built for is held on the CPU (tests/test_lz4_payload_grid.py)."""
import numpy as np
import pytest

import lz4_payload_grid as G
from test_device_lz4 import _chunks, _lz4_decompress

pytestmark = pytest.mark.gpu

_models = {}


def _model_blocks(oracle, stage2, case):
    """per cloud of the case: [(payload, the model's block)] of its chunks (computed once, shared by the orders and tests)"""
    key = (stage2, case.id)
    if key not in _models:
        _models[key] = [[(p, oracle.lz4_model(p, *G.PARAMS[stage2])) for p in G.chunk_payloads(case.schema, cloud)] for cloud in case.clouds]
    return _models[key]


@pytest.mark.parametrize("stage2", [1, 2])
@pytest.mark.parametrize("family,schema_name", G.BATCH_KEYS, ids=[f"{f}-{s}" for f, s in G.BATCH_KEYS])
def test_grid_blocks_equal_the_model_and_decode(oracle, family, schema_name, stage2):
    from cloudini_amd import native
    batch = G.batches(stage2)[(family, schema_name)]
    info = G.schema(schema_name)
    step = G.STEPS[schema_name]
    codec = native.Codec(native.Plan(info))
    for order in (batch, batch[::-1]):
        items = [(c, k) for c in order for k in range(len(c.clouds))]
        clouds = [c.clouds[k] for c, k in items]
        codec.set_stage2(0)
        plain, plain_sizes, _ = codec.encode_host(clouds)
        codec.set_stage2(stage2)
        streams, chunk_sizes, _ = codec.encode_host(clouds)
        assert len(streams) == len(plain) == len(clouds)
        pos = 0
        for (c, k), cloud, s1, stream in zip(items, clouds, plain, streams):
            assert np.array_equal(s1, oracle.encode_stage1(info, cloud)), c.id
            want = _model_blocks(oracle, stage2, c)[k]
            payloads, blocks = _chunks(s1), _chunks(stream)                   # (_chunks: the size prefixes add up to the stream)
            assert len(payloads) == len(blocks) == len(want), c.id
            for j, (payload, block, (raw, model)) in enumerate(zip(payloads, blocks, want)):
                assert np.array_equal(payload, raw), (c.id, j)                # the compressor was handed the grid's bytes
                assert int(plain_sizes[pos]) == payload.size and int(chunk_sizes[pos]) == block.size, (c.id, j)
                pos += 1
                assert block.size == model.size, (c.id, j, block.size, model.size)
                assert np.array_equal(block, model), (c.id, j, int(np.nonzero(block != model)[0][0]))
                assert _lz4_decompress(np.ascontiguousarray(block), raw.size) == raw.tobytes(), (c.id, j)
        assert pos == len(chunk_sizes) == len(plain_sizes)
        out = np.full(sum(cl.size for cl in clouds), 0xA5, dtype=np.uint8)
        back = codec.decode_lz4_host(streams, [cl.size // step for cl in clouds], out=out)
        for (c, _k), cloud, got in zip(items, clouds, back):
            assert np.array_equal(got, cloud), c.id
    codec.close()


@pytest.mark.parametrize("stage2", [1, 2])
@pytest.mark.parametrize("schema_name", ["RAW4", "RAW32"])
def test_span_threshold_at_every_output_alignment(oracle, schema_name, stage2):
    """Family i through encode_device with `out` at 0, 1, 7 and 15 bytes from a 256-byte aligned buffer prefilled with 0xA5:
    the model's bytes at every offset, nothing written in front of `out` or behind the reported total. With the addresses known
    the trace tells which path sub-range 0 of every case took: both paths are taken, and a case whose span is 7 bytes below
    the image (x = 314) takes one path at some of the four offsets and the other at the rest."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    sub = G.PARAMS[stage2][0]
    k_img = sub + G.K_IMG_EXTRA
    batch = G.batches(stage2)[("i", schema_name)]
    info = G.schema(schema_name)
    step = G.STEPS[schema_name]
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    codec.set_stage2(stage2)
    clouds = [c.clouds[0] for c in batch]
    npts = np.array([cl.size // step for cl in clouds], dtype=np.uint64)
    cap = int(sum(plan.stage2_bound(int(n), stage2) for n in npts))
    wants, spans = [], []
    for c in batch:
        (payload, model), = _model_blocks(oracle, stage2, c)[0]                # one chunk each
        wants.append(np.concatenate([np.array([model.size], dtype="<u4").view(np.uint8), model]))
        r = oracle.lz4_trace(payload, *G.PARAMS[stage2]).subs[0]
        spans.append((int(r["w0"]), int(r["span"])))
    want = np.concatenate(wants)
    want_offs = np.concatenate([[0], np.cumsum([w.size for w in wants])]).astype(np.uint64)
    d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
    front = 256
    direct = {c.id: [] for c in batch}
    for off in (0, 1, 7, 15):
        d_out = torch.full((front + 16 + cap + 256,), 0xA5, dtype=torch.uint8, device=dev)
        assert d_out.data_ptr() % 256 == 0
        d_off = torch.zeros(len(clouds) + 1, dtype=torch.int64, device=dev)
        d_sizes = torch.zeros(len(clouds), dtype=torch.int32, device=dev)
        out_ptr = d_out.data_ptr() + front + off
        codec.encode_device(d_in.data_ptr(), npts, out_ptr, cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
        codec.synchronize()
        codec.status()
        host = d_out.cpu().numpy()
        offs = d_off.cpu().numpy().astype(np.uint64)
        assert np.array_equal(offs, want_offs), off
        assert [int(x) + 4 for x in d_sizes.cpu().numpy()] == [w.size for w in wants], off
        total = int(offs[-1])
        assert (host[:front + off] == 0xA5).all(), off                           # nothing in front of `out`
        assert (host[front + off + total:] == 0xA5).all(), off                   # nothing behind the reported total
        got = host[front + off:front + off + total]
        for c, a, b in zip(batch, want_offs[:-1], want_offs[1:]):
            assert np.array_equal(got[int(a):int(b)], want[int(a):int(b)]), (c.id, off)
        for c, a, (w0, span) in zip(batch, want_offs[:-1], spans):               # k_lz4_emit_lds: pad = (out + W0) & 15
            pad = (out_ptr + int(a) + 4 + w0) & 15
            direct[c.id].append(span + pad > k_img)
    codec.close()
    taken = [d for ds in direct.values() for d in ds]
    assert any(taken) and not all(taken)
    for c in batch:
        if c.name.endswith("_x314"):
            assert any(direct[c.id]) and not all(direct[c.id]), (c.id, direct[c.id])
