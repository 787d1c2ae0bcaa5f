"""Device-resident calls on a busy caller stream, back to back (include/cloudini_hip.h: "with DEVICE pointers a call only
enqueues work on the codec's HIP stream").

One run is a sequence of calls on one codec and one stream with no host synchronisation of the test's own between the first
enqueue and the last. In front of every call the stream is held by a delay; behind the hold a copy on the same stream puts
the call's true input over a decoy (another valid input of the same size), and right behind the call copies on the same
stream snapshot everything it hands out. Work the library issued on any other stream, or a host step it took too early,
meets the decoy or a sentinel: wrong bytes, nothing worse. After the last call: one stream synchronise, one status(), and
the snapshots, the buffers and the guard bytes around them against the oracle (plans: tests/stream_order_cases.py).
Every case runs on a stream of the caller's and on the codec's own."""
import threading

import numpy as np
import pytest

import stream_order_cases as S

pytestmark = pytest.mark.gpu

SENT = 0xC7
GUARD = 256
KINDS = ["caller_stream", "own_stream"]
HOLD_MS = 30.0          # aimed at; a hold of 20 to 40 ms is long against a call's launch and enqueue cost (about 50 us of device time)
FACTS = {"hold_ms": None, "lookback_timeouts": 0}


def _measure(torch, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="module")
def hold():
    """cycles of torch.cuda._sleep for a hold of about HOLD_MS, calibrated once with two events"""
    import torch
    _measure(torch, 1000000)
    probe = 20000000
    cycles = max(1, int(probe * HOLD_MS / max(1e-3, _measure(torch, probe))))
    ms = _measure(torch, cycles)
    FACTS["hold_ms"] = ms
    print(f"\nstream-order hold: {cycles} cycles measure {ms:.1f} ms")
    assert ms >= 10.0, f"the calibrated hold lasts {ms:.2f} ms: too short to keep a stream busy across a call's enqueue"
    return cycles


# ---- buffers ---------------------------------------------------------------------------------------------------------
def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Out:
    """`nbytes` of device memory a call writes, `odd` bytes behind a 256-byte boundary, between guard spans, all pre-filled with
    the sentinel; and the tensor a copy behind the call snapshots it into."""

    def __init__(self, nbytes, odd=0):
        import torch
        dev = torch.device("cuda", 0)
        self.t = torch.full((256 + GUARD + 16 + nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.at = (-self.t.data_ptr()) % 256 + GUARD + odd
        self.n = nbytes
        self.ptr = self.t.data_ptr() + self.at
        self.snap = torch.full_like(self.t, 0x11)

    def snapshot(self):
        self.snap.copy_(self.t, non_blocking=True)

    def check(self, what, want=None, exact=True, loose=None):
        """Snapshot and buffer: the guards hold the sentinel, the first want.size bytes are `want` (loose: bytes that may
        also be 0), the rest of the span holds the sentinel if `exact`."""
        want = np.zeros(0, np.uint8) if want is None else _u8(want)
        for name, t in (("snapshot", self.snap), ("buffer", self.t)):
            host = t.cpu().numpy()
            assert (host[:self.at] == SENT).all() and (host[self.at + self.n:] == SENT).all(), (what, name, "bytes around the output")
            got = host[self.at:self.at + want.size]
            if loose is not None:
                assert ((got[loose] == SENT) | (got[loose] == 0)).all(), (what, name, "bytes no field covers")
                got, w = got[~loose], want[~loose]
            else:
                w = want
            if not np.array_equal(got, w):
                bad = np.nonzero(got != w)[0]
                raise AssertionError((what, name, "%d of %d bytes differ, the first at %d" % (bad.size, w.size, int(bad[0]))))
            if exact:
                assert (host[self.at + want.size:self.at + self.n] == SENT).all(), (what, name, "bytes behind the output")


class Inp:
    """A call's input: it holds `decoy` until produce() -- a device-to-device copy on the current stream -- writes `true`."""

    def __init__(self, true, decoy=None, odd=0):
        import torch
        dev = torch.device("cuda", 0)
        true = _u8(true)
        decoy = true if decoy is None else _u8(decoy)
        assert true.size == decoy.size
        self.n = true.size
        self.t = torch.zeros(256 + 16 + self.n + 64, dtype=torch.uint8, device=dev)
        at = (-self.t.data_ptr()) % 256 + odd
        self.view = self.t[at:at + self.n]
        self.ptr = self.t.data_ptr() + at
        self.src = torch.from_numpy(true.copy()).to(dev) if self.n else None
        self.true = true
        if self.n:
            self.view.copy_(torch.from_numpy(decoy.copy()).to(dev))

    def produce(self):
        if self.n:
            self.view.copy_(self.src, non_blocking=True)

    def check(self, what):
        assert np.array_equal(self.view.cpu().numpy(), self.true), (what, "an input buffer has changed")


class Step:
    def __init__(self, what, call, inputs=(), outs=(), verify=None):
        self.what, self.call, self.inputs, self.outs, self.verify = what, call, list(inputs), list(outs), verify


class Run:
    """One codec, one stream, a list of steps."""

    def __init__(self, info, kind, hold, setup=None):
        import torch
        from cloudini_amd import native
        self.torch, self.native, self.info, self.hold = torch, native, info, hold
        self.plan = native.Plan(info)
        if kind == "caller_stream":
            self.stream = torch.cuda.Stream()
            self.codec = native.Codec(self.plan, device=0, stream=self.stream.cuda_stream)
            assert self.codec.stream() == self.stream.cuda_stream
        else:
            self.codec = native.Codec(self.plan, device=0)
            assert self.codec.stream() != 0
            self.stream = torch.cuda.ExternalStream(self.codec.stream())
        if setup:
            setup(self.codec)
        self.steps = []

    def add(self, *a, **kw):
        self.steps.append(Step(*a, **kw))
        return self.steps[-1]

    def enqueue(self, step):
        """on the current stream: the hold, the producers, the call, the snapshots"""
        self.torch.cuda._sleep(self.hold)
        for i in step.inputs:
            i.produce()
        step.call()
        for o in step.outs:
            o.snapshot()

    def go(self, expect_error=None):
        torch = self.torch
        torch.cuda.synchronize()                 # every fill has landed: none can race a call
        with torch.cuda.stream(self.stream):
            for step in self.steps:
                self.enqueue(step)
        self.stream.synchronize()
        if expect_error is None:
            self.codec.status()
        else:
            with pytest.raises(self.native.CloudiniHipError) as e:
                self.codec.status()
            assert e.value.code == expect_error, e.value
        self.check()

    def check(self):
        for step in self.steps:
            for i in step.inputs:
                i.check(step.what)
            if step.verify:
                step.verify()

    def close(self):
        self.codec.close()


# ---- the calls -------------------------------------------------------------------------------------------------------
def _cat(clouds, pad=0):
    return np.concatenate([_u8(c) for c in clouds] + [np.zeros(pad, np.uint8)])


def add_encode(run, oracle, k, clouds, decoys, via="framed", plain=False, want=None, stage2=0, judge=None):
    """One encode call of `clouds` (the input holds `decoys` until the producer runs) against the oracle. k varies what the
    call is given: the modes pointer or 0, stream_offsets and chunk_sizes or 0, odd addresses. via: "framed" (encode_device) or
    "chunks" (encode_chunks_device, then frame_chunks_device as a step of its own). plain: everything given, aligned."""
    info, plan, codec = run.info, run.plan, run.codec
    want = S.want_encode(oracle, info, clouds) if want is None else want
    counts = want.counts
    n_chunks = S.n_chunks_of(counts)
    na = want.modes.shape[1] if want.modes.size else plan.adaptive_fields
    inp = Inp(_cat(clouds), _cat(decoys), odd=0 if plain else (0, 4, 1, 0, 7, 2)[k % 6])
    cap = max(16, sum(plan.stage2_bound(int(n), stage2) for n in counts))
    give_modes = plain or k % 3 != 1
    give_off = plain or k % 4 != 3
    give_sizes = plain or k % 5 != 2
    out = Out(cap, odd=0 if plain else (0, 1, 0, 3, 0, 7)[k % 6])
    off = Out(8 * (len(clouds) + 1), odd=0 if plain or k % 7 != 3 else 4) if give_off else None
    sizes = Out(4 * max(1, n_chunks), odd=0 if plain or k % 7 != 5 else 2) if give_sizes else None
    modes = Out(max(1, len(clouds) * na), odd=0 if plain else k % 4) if give_modes else None
    outs = [o for o in (out, off, sizes, modes) if o is not None]
    what = ("encode", via, k)

    def verify():
        if judge is not None:
            judge(what, out, off, sizes, want)
        else:
            out.check(what + ("streams",), want.bytes, exact=False)
            if off is not None:
                off.check(what + ("stream_offsets",), want.offsets)
            if sizes is not None:
                sizes.check(what + ("chunk_sizes",), want.sizes, exact=n_chunks > 0)
        if modes is not None:
            modes.check(what + ("modes",), want.modes, exact=want.modes.size > 0)

    if via == "framed":
        run.add(what, lambda: codec.encode_device(inp.ptr, counts, out.ptr, cap, off.ptr if off else 0, sizes.ptr if sizes else 0,
                                                  modes.ptr if modes else 0), [inp], outs, verify)
    else:
        def chunks():
            table = codec.encode_chunks_device(inp.ptr, counts, modes.ptr if modes else 0)
            assert table.n_chunks == n_chunks
        run.add(what, chunks, [inp], [modes] if modes else [])
        run.add(("frame_chunks", k), lambda: codec.frame_chunks_device(out.ptr, cap, off.ptr if off else 0, sizes.ptr if sizes else 0),
                [], [o for o in (out, off, sizes) if o is not None], verify)
    return out, off, sizes, want


def add_decode(run, oracle, k, clouds, wrap=None, fill_zero=False, streams_at=None, sizes_at=None):
    """One decode call: the streams are the oracle's (a decoy stream of the same length until the producer runs), or, with
    streams_at / sizes_at, what an encode call of this run left on the device. chunk_sizes are given for odd k."""
    info, codec = run.info, run.codec
    step = info.point_step
    counts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    pairs = [S.decode_pair(oracle, info, c, wrap) for c in clouds]
    offs = np.concatenate([[0], np.cumsum([p[0].size for p in pairs])]).astype(np.uint64)
    inputs = []
    if streams_at is None:
        inp = Inp(_cat([p[0] for p in pairs]), _cat([p[1] for p in pairs]), odd=k % 3)
        inputs.append(inp)
        streams_at = inp.ptr
    sized = None
    if wrap is None and sizes_at is None and k % 2 == 1 and S.n_chunks_of(counts):
        sized = Inp(np.array([q.size for p in pairs for q in S.chunk_payloads(p[0])], dtype=np.uint32))
        inputs.append(sized)
        sizes_at = sized.ptr
    out = Out(int(counts.sum()) * step, odd=(0, 5, 2, 15)[k % 4])
    want = _cat([S.want_decode(oracle, info, c, SENT) for c in clouds])
    loose = np.tile(~S.covered_mask(info), int(counts.sum())) if fill_zero else None
    fn = {None: None, S.lz4_body_of: codec.decode_lz4_device, S.zstd_body_of: codec.decode_zstd_device}[wrap]

    def call():
        codec.set_decode_fill(fill_zero)
        if fn is None:
            codec.decode_device(streams_at, offs, counts, out.ptr, out.n, sizes_at or 0)
        else:
            fn(streams_at, offs, counts, out.ptr, out.n)
    what = ("decode", k)
    run.add(what, call, inputs, [out], lambda: out.check(what, want, loose=loose))
    return out


def _pairs(plan):
    return [(S.clouds_of(c), S.decoys_of(c)) for c in plan]


# ---- 1. encode_device, both pipelines; the two other schemas ------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pipeline", [2, 1])
def test_encode_main_plan(oracle, hold, kind, pipeline):
    run = Run(S.INFO, kind, hold, lambda codec: codec.pipeline(pipeline))
    for k, (clouds, decoys) in enumerate(_pairs(S.MAIN_PLAN)):
        add_encode(run, oracle, k, clouds, decoys)
    run.go()
    assert run.codec.finish_retries() == 0
    run.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("schema", ["ouster_like", "very_wide"])
def test_encode_and_decode_of_the_other_schemas(oracle, hold, kind, schema):
    """A Gorilla field (the call uploads its pre-pass pointers and waits) and the WIDE route: plain encode calls, then the same
    clouds back through plain decode calls, one codec."""
    info, calls, decoys = S.ouster_calls() if schema == "ouster_like" else S.wide_calls()
    run = Run(info, kind, hold)
    for k, (clouds, dec) in enumerate(zip(calls, decoys)):
        add_encode(run, oracle, k, clouds, dec, plain=k % 2 == 0)
    for k, clouds in enumerate(calls):
        add_decode(run, oracle, k, clouds)
    run.go()
    run.close()


# ---- 2. chunk table, then framing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_chunk_table_and_framing_as_pairs(oracle, hold, kind):
    run = Run(S.INFO, kind, hold)
    for k, (clouds, decoys) in enumerate(_pairs(S.MAIN_PLAN)):
        add_encode(run, oracle, k, clouds, decoys, via="chunks")
    run.go()
    run.close()


# ---- 3. stage 2 on the device ---------------------------------------------------------------------------------------------
def _judge_stage2(decompress):
    """as tests/test_gpu_lz4_encode_grid.py and tests/test_gpu_zstd_encode.py judge: every chunk, decompressed by the system's
    library, is the oracle's payload; offsets and sizes describe the blocks"""
    def judge(what, out, off, sizes, want):
        payloads = [p for s in want.streams for p in S.chunk_payloads(s)]
        for name, t_out, t_off, t_sizes in (("snapshot", out.snap, off.snap, sizes.snap), ("buffer", out.t, off.t, sizes.t)):
            out.check(what, exact=False)
            off.check(what, exact=False)
            sizes.check(what, exact=False)
            offs = t_off.cpu().numpy()[off.at:off.at + off.n].view("<u8")
            got_sizes = t_sizes.cpu().numpy()[sizes.at:sizes.at + 4 * len(payloads)].view("<u4")
            body = t_out.cpu().numpy()[out.at:out.at + out.n]
            assert int(offs[0]) == 0 and int(offs[-1]) <= out.n, (what, name)
            j = 0
            for c, s in enumerate(want.streams):
                blocks = S.chunk_payloads(body[int(offs[c]):int(offs[c + 1])])
                assert len(blocks) == len(S.chunk_payloads(s)), (what, name, c)
                for block in blocks:
                    assert int(got_sizes[j]) == block.size, (what, name, c, j)
                    assert decompress(np.ascontiguousarray(block), payloads[j].size) == payloads[j].tobytes(), (what, name, c, j)
                    j += 1
            assert j == len(payloads)
    return judge


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stage2", ["lz4", "lz4_fast", "zstd", "zstd_matches"])
def test_encode_with_stage2_on_the_device(oracle, hold, kind, stage2):
    from test_device_lz4 import _lz4_decompress
    from test_zstd_lit_model import zstd_decompress
    mode = {"lz4": 1, "lz4_fast": 2, "zstd": 3, "zstd_matches": 3}[stage2]

    def setup(codec):
        codec.set_stage2(mode)
        if stage2 == "zstd_matches":
            codec.set_zstd_matches(True)
    run = Run(S.INFO, kind, hold, setup)
    judge = _judge_stage2(_lz4_decompress if mode < 3 else (lambda block, size: zstd_decompress(block.tobytes(), size)))
    for k, (clouds, decoys) in enumerate(_pairs(S.STAGE2_PLAN)):
        add_encode(run, oracle, k, clouds, decoys, plain=True, stage2=mode, judge=judge)
    run.go()
    run.close()


# ---- 4. decode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fill_zero", [False, True])
def test_decode_plan(oracle, hold, kind, fill_zero):
    run = Run(S.INFO, kind, hold)
    for k, call in enumerate(S.DECODE_PLAN):
        add_decode(run, oracle, k, S.clouds_of(call), fill_zero=fill_zero)
    run.go()
    run.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stage2", ["lz4", "zstd"])
def test_decode_of_host_library_bodies(oracle, hold, kind, stage2):
    wrap = S.lz4_body_of if stage2 == "lz4" else S.zstd_body_of
    run = Run(S.INFO, kind, hold, (lambda codec: codec.set_zstd_sequences(True)) if stage2 == "zstd" else None)
    for k, call in enumerate(S.STAGE2_DECODE_PLAN):
        add_decode(run, oracle, k, S.clouds_of(call), wrap=wrap, fill_zero=k % 2 == 1)
    run.go()
    run.close()


# ---- 5. round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_pairs(oracle, hold, kind):
    """encode_device, then decode_device of what it wrote: offsets from the oracle, chunk sizes from the encode call's device array"""
    run = Run(S.INFO, kind, hold)
    assert len(S.ROUND_TRIP_PLAN) >= 12
    for k, (clouds, decoys) in enumerate(_pairs(S.ROUND_TRIP_PLAN)):
        out, _off, sizes, _want = add_encode(run, oracle, k, clouds, decoys, plain=True)
        add_decode(run, oracle, k, clouds, streams_at=out.ptr, sizes_at=sizes.ptr if S.n_chunks_of(S.shape_of(S.ROUND_TRIP_PLAN[k])) else None)
    run.go()
    run.close()


# ---- 6. reports ----------------------------------------------------------------------------------------------------------------
def _report_steps(run, oracle, seed0=0):
    """The report calls with DEVICE reports, another batch for each: [(name, add)] -- add() appends the step(s) to the run."""
    import audit_model as AM
    import hist_model as HM
    import mode_model as MM
    import sweep_model as SM
    info, codec = S.INFO, run.codec
    ladders = SM.default_ladders(info, (1.0, 0.5))

    def batch(j, shape):
        specs = [((j + k) % 4, n, 300 + seed0 + 8 * j + k) if n >= 300 else (None, n, 300 + seed0 + 8 * j + k) for k, n in enumerate(shape)]
        return [S.cloud_of(s) for s in specs], [S.decoy_of(s) for s in specs], np.array(shape, dtype=np.uint64)

    def decoded(clouds):
        return [S.want_decode(oracle, info, c, 0) for c in clouds]

    def audit_clouds():
        clouds, decoys, counts = batch(0, [1025, 0, 2049])
        a, b = Inp(_cat(clouds), _cat(decoys), odd=7), Inp(_cat(decoded(clouds)), odd=3)
        want = AM.audit(info, _cat(clouds), _cat(decoded(clouds)), counts)
        rep = Out(want.nbytes)
        what = ("audit_clouds",)
        run.add(what, lambda: codec.audit_clouds_device(a.ptr, b.ptr, counts, report_ptr=rep.ptr), [a, b], [rep],
                lambda: rep.check(what, want))

    def sweep_clouds():
        clouds, decoys, counts = batch(1, [700, 4097])
        p = Inp(_cat(clouds), _cat(decoys), odd=1)
        want = SM.sweep(info, _cat(clouds), counts, ladders)
        rep = Out(want.nbytes)
        what = ("sweep_clouds",)
        run.add(what, lambda: codec.sweep_clouds_device(p.ptr, counts, ladders, report_ptr=rep.ptr), [p], [rep],
                lambda: rep.check(what, want))

    def audit_streams():
        clouds, decoys, counts = batch(2, [3000, 1, 300])
        w = S.want_encode(oracle, info, clouds)
        p, s = Inp(_cat(clouds), _cat(decoys), odd=5), Inp(w.bytes, odd=2)
        want = AM.audit(info, _cat(clouds), _cat(decoded(clouds)), counts)
        rep = Out(want.nbytes)
        what = ("audit_streams",)
        run.add(what, lambda: codec.audit_streams_device(p.ptr, s.ptr, w.offsets, counts, report_ptr=rep.ptr), [p, s], [rep],
                lambda: rep.check(what, want))

    def sweep_hist():
        clouds, decoys, counts = batch(3, [1500, 301])
        p = Inp(_cat(clouds), _cat(decoys), odd=9)
        want = HM.sweep_hist(info, _cat(clouds), counts, ladders)
        rep = Out(want.nbytes)
        what = ("sweep_hist_clouds",)
        run.add(what, lambda: codec.sweep_hist_clouds_device(p.ptr, counts, ladders, report_ptr=rep.ptr), [p], [rep], lambda: rep.check(what, want))

    def stream_hist():
        clouds, _decoys, _counts = batch(4, [2000, 0, 310])
        pairs = [S.decode_pair(oracle, info, c) for c in clouds]
        offs = np.concatenate([[0], np.cumsum([q[0].size for q in pairs])]).astype(np.uint64)
        s = Inp(_cat([q[0] for q in pairs]), _cat([q[1] for q in pairs]), odd=11)
        want = HM.stream_hist([q[0] for q in pairs])
        rep = Out(want.nbytes)
        what = ("stream_hist",)
        run.add(what, lambda: codec.stream_hist_device(s.ptr, offs, report_ptr=rep.ptr), [s], [rep], lambda: rep.check(what, want))

    def sweep_modes():
        clouds, decoys, counts = batch(5, [1, 0, 4097, 5000, 63])
        p = Inp(_cat(clouds), _cat(decoys), odd=7)
        want = MM.sweep(info, _cat(clouds), counts)
        rep = Out(want.nbytes)
        what = ("sweep_modes",)
        run.add(what, lambda: codec.sweep_modes_device(p.ptr, counts, report_ptr=rep.ptr), [p], [rep], lambda: rep.check(what, want))

    def last_encode(which, j):
        def add():
            clouds, decoys, counts = batch(6 + j, [[2100, 300], [301, 0, 1700], [3333], [640, 2000]][j])
            add_encode(run, oracle, 0, clouds, decoys, plain=True)
            w = S.want_encode(oracle, info, clouds)
            for name in which:
                what = (name, j)
                if name == "audit_last_encode":
                    want = AM.audit(info, _cat(clouds), _cat(decoded(clouds)), counts)
                    rep = Out(want.nbytes)
                    run.add(what, lambda rep=rep: codec.audit_last_encode(report_ptr=rep.ptr), [], [rep],
                            lambda rep=rep, want=want, what=what: rep.check(what, want))
                elif name == "sweep_last_encode":
                    want = SM.sweep(info, _cat(clouds), counts, ladders)
                    rep = Out(want.nbytes)
                    run.add(what, lambda rep=rep: codec.sweep_last_encode(ladders, report_ptr=rep.ptr), [], [rep],
                            lambda rep=rep, want=want, what=what: rep.check(what, want))
                elif name == "stream_hist_last_encode":
                    want = HM.stream_hist(w.streams)
                    rep = Out(want.nbytes)
                    run.add(what, lambda rep=rep: codec.stream_hist_last_encode(report_ptr=rep.ptr), [], [rep],
                            lambda rep=rep, want=want, what=what: rep.check(what, want))
                elif name == "sweep_hist_last_encode":
                    want = HM.sweep_hist(info, _cat(clouds), counts, ladders)
                    rep = Out(want.nbytes)
                    run.add(what, lambda rep=rep: codec.sweep_hist_last_encode(ladders, report_ptr=rep.ptr), [], [rep],
                            lambda rep=rep, want=want, what=what: rep.check(what, want))
                else:
                    want = MM.sweep(info, _cat(clouds), counts)
                    rep = Out(want.nbytes)
                    run.add(what, lambda rep=rep: codec.sweep_modes_last_encode(report_ptr=rep.ptr), [], [rep],
                            lambda rep=rep, want=want, what=what: rep.check(what, want))
        return add

    return {"audit_clouds": audit_clouds, "sweep_clouds": sweep_clouds, "audit_streams": audit_streams, "sweep_hist": sweep_hist,
            "stream_hist": stream_hist, "sweep_modes": sweep_modes,
            "last_a": last_encode(["sweep_last_encode", "audit_last_encode"], 0),
            "last_b": last_encode(["stream_hist_last_encode", "sweep_hist_last_encode", "sweep_modes_last_encode", "audit_last_encode"], 1),
            "last_c": last_encode(["audit_last_encode"], 2), "last_d": last_encode(["sweep_modes_last_encode", "stream_hist_last_encode"], 3)}


@pytest.mark.parametrize("kind", KINDS)
def test_report_calls_interleaved(oracle, hold, kind):
    run = Run(S.INFO, kind, hold)
    steps = _report_steps(run, oracle)
    for name in ("audit_clouds", "sweep_clouds", "last_a", "audit_streams", "sweep_hist", "stream_hist", "last_b", "sweep_modes",
                 "audit_clouds", "last_d", "sweep_clouds", "last_c"):
        steps[name]()
    assert len(run.steps) >= 20
    run.go()
    run.close()


# ---- 7. mixed ---------------------------------------------------------------------------------------------------------------
def add_viz(run, oracle, k, clouds, decoys):
    """encode_viz_device: the filter's counts come back on the host (the call waits for them), the rest as an encode call of the
    survivors"""
    info, plan, codec = run.info, run.plan, run.codec
    surv, want = S.want_viz(oracle, clouds)
    counts = np.array([c.size // info.point_step for c in clouds], dtype=np.uint64)
    inp = Inp(_cat(clouds), _cat(decoys), odd=k % 5)
    cap = max(16, sum(plan.stage1_bound(int(n)) for n in counts))
    out, off, sizes, modes = Out(cap, odd=k % 3), Out(8 * (len(clouds) + 1)), Out(4 * max(1, S.n_chunks_of(counts))), Out(len(clouds))
    what = ("encode_viz", k)

    def call():
        kept = codec.encode_viz_device(inp.ptr, counts, 0, S.VIZ_RESOLUTION, out.ptr, cap, off.ptr, sizes.ptr, modes.ptr)
        assert [int(x) for x in kept] == [int(x) for x in want.counts], (what, "kept_points")

    def verify():
        out.check(what + ("streams",), want.bytes, exact=False)
        off.check(what + ("stream_offsets",), want.offsets)
        sizes.check(what + ("chunk_sizes",), want.sizes, exact=False)
        modes.check(what + ("modes",), want.modes)
    assert 0 < sum(int(x) for x in want.counts) < int(counts.sum())      # the filter drops points and keeps some
    run.add(what, call, [inp], [out, off, sizes, modes], verify)


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_calls_share_one_codec(oracle, hold, kind):
    """Framed encodes, chunk tables, decodes, reports and viz encodes in one sequence: they share d_status, d_in and the workspaces."""
    run = Run(S.INFO, kind, hold)
    reports = _report_steps(run, oracle, seed0=100)
    main = _pairs(S.MAIN_PLAN)
    enc = lambda k, via="framed": (lambda: add_encode(run, oracle, k, main[k][0], main[k][1], via=via))
    dec = lambda k, j: (lambda: add_decode(run, oracle, k, S.clouds_of(S.DECODE_PLAN[j]), fill_zero=k % 2 == 0))
    viz = lambda k, call: (lambda: add_viz(run, oracle, k, S.clouds_of(call), S.decoys_of(call)))
    plan = [enc(0), dec(0, 1), enc(2, "chunks"), reports["audit_clouds"], enc(4), dec(1, 0), viz(0, [(None, 20000, 400), (None, 300, 401)]),
            reports["sweep_clouds"], enc(6), enc(7), dec(2, 3), enc(8, "chunks"), reports["stream_hist"], enc(9), dec(3, 7),
            reports["sweep_modes"], enc(10), dec(4, 5), viz(1, [(None, 40000, 402)]), enc(11), reports["last_c"], dec(5, 9),
            enc(12, "chunks"), reports["audit_streams"], enc(13), dec(6, 2), reports["sweep_hist"], enc(1)]
    for add in plan:
        add()
    assert len(run.steps) >= 24
    run.go()
    assert run.codec.finish_retries() == 0
    run.close()


# ---- 8. wire version 2: one unframed run of points ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", S.UNFRAMED_N)
def test_unframed_payloads(oracle, hold, kind, n):
    """Capacities: exact, 500 points more (the tail keeps the sentinel), one point short (CORRUPT, read with status())."""
    info = S.UNFRAMED_INFO
    step = info.point_step
    payload, decoy, cloud = S.unframed_case(oracle, n)
    want = oracle.decode_stage1(info, np.concatenate([np.frombuffer(np.uint32(payload.size).tobytes(), np.uint8), payload]), n, fill=SENT)

    def add(run, k, points):
        inp, out = Inp(payload, decoy, odd=k), Out(points * step, odd=(0, 3, 6)[k])
        what = ("unframed", n, points)
        run.add(what, lambda: run.codec.decode_unframed_device(inp.ptr, payload.size, out.ptr, out.n), [inp], [out],
                (lambda: out.check(what, want)) if points >= n else (lambda: out.check(what, exact=False)))
    run = Run(info, kind, hold)
    add(run, 0, n)
    add(run, 1, n + S.UNFRAMED_EXTRA)
    add(run, 2, n)
    run.go()
    run.steps = []
    add(run, 0, n + S.UNFRAMED_EXTRA)
    add(run, 1, n)
    add(run, 2, n - 1)
    run.go(expect_error=-6)
    run.close()


# ---- 9. a bad call in mid-run -------------------------------------------------------------------------------------------------
def _add_damaged(run, oracle):
    stream, n = S.chunk_missing(oracle)
    inp, out = Inp(stream), Out(n * 16)
    offs, counts = np.array([0, stream.size], dtype=np.uint64), np.array([n], dtype=np.uint64)
    what = ("decode", "chunk_missing")
    run.add(what, lambda: run.codec.decode_device(inp.ptr, offs, counts, out.ptr, out.n), [inp], [out], lambda: out.check(what, exact=False))


@pytest.mark.parametrize("kind", KINDS)
def test_a_damaged_stream_in_mid_run_and_at_the_end(oracle, hold, kind):
    """status() reports the last asynchronous call: behind a refused stream in the middle every later call still gives the
    oracle's points and the status is OK; with the refused stream last it is CORRUPT."""
    run = Run(S.INFO, kind, hold)
    plan = S.DECODE_PLAN[:8]
    for k, call in enumerate(plan):
        if k == 4:
            _add_damaged(run, oracle)
        add_decode(run, oracle, k, S.clouds_of(call))
    run.go()
    run.steps = []
    for k, call in enumerate(plan[:4]):
        add_decode(run, oracle, k + 1, S.clouds_of(call))
    _add_damaged(run, oracle)
    run.go(expect_error=-6)
    run.close()


# ---- the self-check: a mis-ordered read shows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_hold_on_a_side_stream_orders_nothing_on_the_codecs_stream(oracle, hold, kind):
    """The hold and the producer on a SIDE stream, nothing in front of the call on the codec's stream: the call reads the decoy,
    and the comparison sees it -- the oracle's bytes for the decoy, not for the cloud the producer writes later."""
    import torch
    run = Run(S.INFO, kind, hold)
    clouds, decoys = S.clouds_of(S.MAIN_PLAN[6]), S.decoys_of(S.MAIN_PLAN[6])
    warm = S.clouds_of(S.MAIN_PLAN[7])
    add_encode(run, oracle, 0, warm, warm, plain=True)         # (the workspaces are allocated, the batch shape is uploaded)
    run.go()
    run.steps = []
    w_true, w_decoy = S.want_encode(oracle, S.INFO, clouds), S.want_encode(oracle, S.INFO, decoys)
    assert not np.array_equal(w_true.bytes, w_decoy.bytes) and not np.array_equal(w_true.modes, w_decoy.modes)
    add_encode(run, oracle, 0, clouds, decoys, plain=True, want=w_decoy)
    step = run.steps[0]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(3):
            torch.cuda._sleep(hold)
        for i in step.inputs:
            i.produce()
    with torch.cuda.stream(run.stream):
        step.call()
        for o in step.outs:
            o.snapshot()
    torch.cuda.synchronize()
    run.codec.status()
    run.check()          # the outputs are the decoy's; the input buffer holds the true cloud by now: the producer did run
    run.close()


# ---- two codecs at once -----------------------------------------------------------------------------------------------------------
def _finish(run):
    """stream synchronise and status() where k_finish's bounded look-back may report its timeout (include/cloudini_hip.h:
    ERR_DEVICE, "repeat the call", device outputs are never redone by the library): the last call is then repeated once."""
    run.stream.synchronize()
    try:
        run.codec.status()
    except run.native.CloudiniHipError as e:
        if e.code != -4 or "waited too long" not in e.message:
            raise
        FACTS["lookback_timeouts"] += 1
        print("\nstream-order: k_finish reported its look-back timeout; the call is repeated once")
        step = run.steps[-1]
        with run.torch.cuda.stream(run.stream):
            step.call()
            for o in step.outs:
                o.snapshot()
        run.stream.synchronize()
        run.codec.status()
    run.check()


@pytest.mark.parametrize("kind", KINDS)
def test_two_codecs_from_one_thread(oracle, hold, kind):
    """Codec A encodes on stream 1, codec B decodes on stream 2; the enqueues alternate, both streams are held, one
    synchronise at the end."""
    import torch
    a, b = Run(S.INFO, kind, hold), Run(S.INFO, kind, hold)
    n = 10
    for k, (clouds, decoys) in enumerate(_pairs(S.MAIN_PLAN[:n])):
        add_encode(a, oracle, k, clouds, decoys)
    for k, call in enumerate(S.DECODE_PLAN[:n]):
        add_decode(b, oracle, k, S.clouds_of(call))
    torch.cuda.synchronize()
    for sa, sb in zip(a.steps, b.steps):
        with torch.cuda.stream(a.stream):
            a.enqueue(sa)
        with torch.cuda.stream(b.stream):
            b.enqueue(sb)
    _finish(b)
    _finish(a)
    a.close()
    b.close()


def test_two_codecs_from_two_threads(oracle, hold):
    """Each thread creates its own plan, codec and stream behind a barrier (the *_configure* functions of codec_create meet) and
    runs 8 calls of the main plan. One thread makes a host-side ERR_ARG call in the middle; the other thread's
    cldn_hip_last_error() stays empty or its own."""
    import torch
    from cloudini_amd import native
    barrier = threading.Barrier(2)
    pairs = _pairs(S.TWO_THREAD_PLAN)
    for clouds, decoys in pairs:                      # (the oracle's answers are computed once, before the threads start)
        S.want_encode(oracle, S.INFO, clouds)
    errors, seen = {}, {}

    def work(t):
        try:
            torch.cuda.set_device(0)
            barrier.wait(timeout=60)
            run = Run(S.INFO, KINDS[t], hold)
            for k, (clouds, decoys) in enumerate(pairs):
                add_encode(run, oracle, k + t, clouds, decoys)
                if t == 1 and k == 3:
                    def bad():
                        with pytest.raises(native.CloudiniHipError) as e:
                            run.codec.frame_chunks_device(run.steps[0].outs[0].ptr, 1 << 20)      # no chunk table: ERR_ARG, no device work
                        assert e.value.code == -1
                        seen["bad"] = e.value.message
                    run.add(("frame_chunks without a table",), bad)
            torch.cuda.synchronize()
            barrier.wait(timeout=60)
            with torch.cuda.stream(run.stream):
                for step in run.steps:
                    run.enqueue(step)
            seen[t] = native.lib().cldn_hip_last_error().decode(errors="replace")
            _finish(run)
            run.close()
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            errors[t] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in sorted(errors):
        raise errors[t]
    assert seen["bad"] and seen[1] == seen["bad"]       # thread 1 sees its own error text
    assert seen[0] == ""                                # thread 0 made no failing call: its thread-local text is empty
