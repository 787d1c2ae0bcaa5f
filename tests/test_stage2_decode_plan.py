"""The decode direction of the batch transcoder with stage 2 on the device (TranscodeOptions::device_stage2_decode), the parts
that need no GPU:
  * cloudini_amd/csrc/stage2_decode_plan.h -- who undoes stage 2 of a run, and which chunks a second call gets from the host --
    compiled with g++ and checked against a table; the same table through a program of its own under sanitizers;
  * the option's validation in the library and in the command-line tool;
  * the precondition of the "no fall-back" assertions of tests/test_gpu_stage2_decode.py: the device's rule sets, restated in
    tests/zstd_seq_rules.py and tests/lz4_block_rules.py, accept every chunk of the messages those tests build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lz4_block_rules as LR
import lz4_body
import stage2_decode_cases as S
import zstd_seq_rules as ZR
from cloudini_amd.schema import CompressionOption

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloudini_amd", "csrc")
LIB = os.path.join(ROOT, "cloudini_amd", "lib")
NONE, LZ4, ZSTD = 0, 1, 2
HOST_STAGE1, DEVICE_LZ4, DEVICE_ZSTD = 0, 1, 2
NEEDS_HOST, REFUSED = 0xFFFFFFFE, 0xFFFFFFFF

# name -> (option, [(compression, chunks)], [(first, count, first_chunk, n_chunks, call)])
GROUPS = {
    "zstd_on": (True, [(ZSTD, 1), (ZSTD, 3), (ZSTD, 2)], [(0, 3, 0, 6, DEVICE_ZSTD)]),
    "zstd_off": (False, [(ZSTD, 1), (ZSTD, 3), (ZSTD, 2)], [(0, 3, 0, 6, HOST_STAGE1)]),
    # a NONE message inside a batch splits the runs
    "none_inside": (True, [(LZ4, 2), (LZ4, 1), (NONE, 3), (LZ4, 1)], [(0, 2, 0, 3, DEVICE_LZ4), (2, 1, 3, 3, HOST_STAGE1), (3, 1, 6, 1, DEVICE_LZ4)]),
    "mixed": (True, [(NONE, 1), (LZ4, 2), (ZSTD, 3), (ZSTD, 0), (NONE, 1)],
              [(0, 1, 0, 1, HOST_STAGE1), (1, 1, 1, 2, DEVICE_LZ4), (2, 2, 3, 3, DEVICE_ZSTD), (4, 1, 6, 1, HOST_STAGE1)]),
    "empty": (True, [], []),
}
# name -> (return code of the first call: 0 UNSUPPORTED, 1 CORRUPT, 2 ARG, None OK; verdicts; expanded chunks or None = one attempt)
SIZES6 = [100, 200, 300, 400, 500, 600]   # messages of 1, 3 and 2 chunks: chunk 2 is the middle chunk of the middle message
RETRIES = {
    "all_sizes_ok": (None, SIZES6, None),
    "all_sizes_corrupt": (1, SIZES6, None),
    "host_middle": (0, [100, 200, NEEDS_HOST, 400, 500, 600], [2]),
    "refused_middle": (1, [100, 200, REFUSED, 400, 500, 600], [2]),      # the same: the host judges
    "both": (1, [NEEDS_HOST, 200, REFUSED, 400, 500, NEEDS_HOST], [0, 2, 5]),
    "other_error": (2, [NEEDS_HOST, REFUSED], None),
    "empty": (1, [], None),
}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("s2plan") / "libs2plan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "stage2_plan_shim.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    L.plan_groups.argtypes = [C.c_int, u32p, C.c_uint32, u32p, C.c_uint32]
    L.plan_retry.argtypes = [C.c_int, u32p, C.c_uint32, C.POINTER(C.c_uint8)]
    L.plan_retry_fits.argtypes = [C.c_int, u32p, C.c_uint32, u32p, C.c_uint64]
    return L


def _u32(values):
    return (C.c_uint32 * max(1, len(values)))(*values)


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_groups_of_the_first_attempt(shim, name):
    on, msgs, want = GROUPS[name]
    out = (C.c_uint32 * 80)()
    n = shim.plan_groups(1 if on else 0, _u32([x for m in msgs for x in m]), len(msgs), out, 16)
    assert n == len(want)
    assert [tuple(out[5 * k:5 * k + 5]) for k in range(n)] == want


@pytest.mark.parametrize("name", sorted(RETRIES))
def test_chunks_of_the_second_attempt(shim, name):
    code, verdicts, want = RETRIES[name]
    rc = 0 if code is None else shim.plan_codes(code)
    assert code is None or rc < 0
    expanded = (C.c_uint8 * max(1, len(verdicts)))()
    n = shim.plan_retry(rc, _u32(verdicts), len(verdicts), expanded)
    if want is None:
        assert n == -1 and not any(expanded[: len(verdicts)])
    else:
        assert n == len(want) and [c for c in range(len(verdicts)) if expanded[c]] == want


def test_a_host_payload_beyond_the_slot_sends_the_group_to_the_host_route(shim):
    verdicts = [100, NEEDS_HOST, 300]
    rc = shim.plan_codes(0)
    assert shim.plan_retry_fits(rc, _u32(verdicts), 3, _u32([0, 1000, 0]), 1000) == 1
    assert shim.plan_retry_fits(rc, _u32(verdicts), 3, _u32([5000, 1001, 5000]), 1000) == 0   # (only expanded chunks count)
    assert shim.plan_retry_fits(rc, _u32(verdicts), 3, _u32([5000, 1000, 5000]), 1000) == 1


def test_the_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stage2_plan_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stage2_plan_cli.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    got_groups = {l.split()[1]: [tuple(map(int, g.split(":"))) for g in l.split()[2:]] for l in lines if l.startswith("groups ")}
    assert got_groups == {k: v[2] for k, v in GROUPS.items()}
    got_retries = {l.split()[1]: list(map(int, l.split()[2:])) for l in lines if l.startswith("retry ")}
    for name, (_code, verdicts, want) in RETRIES.items():
        flags = [1 if want and c in want else 0 for c in range(len(verdicts))]
        assert got_retries[name] == [1 if want else 0, len(want or [])] + flags, name
    assert lines[-1] == "fits 1 0"


def test_the_option_needs_decode(tmp_path):
    """TranscodeOptions::device_stage2_decode without `decode` is std::invalid_argument, --device-stage2 without --decode exit
    status 2 with a message of its own; --device-zstd with --decode keeps its status."""
    exe = str(tmp_path / "stage2_option_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "stage2_option_check.cpp"), os.path.join(LIB, "libcloudini_amd.so"),
                    os.path.join(LIB, "libcloudini_hip.so"), "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tool = os.path.join(LIB, "cloudini_batch_transcode")
    r = subprocess.run([tool, str(tmp_path / "in"), str(tmp_path / "out"), "--device-stage2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.strip() == "--device-stage2 needs --decode"
    assert not os.path.exists(str(tmp_path / "out"))
    r = subprocess.run([tool, str(tmp_path / "in"), str(tmp_path / "out"), "--decode", "--device-zstd"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--device-zstd is not available with --decode" in r.stderr


@pytest.mark.parametrize("family", S.FAMILIES)
def test_the_rule_sets_accept_every_chunk_of_the_gpu_tests_messages(oracle, family):
    """What tests/test_gpu_stage2_decode.py asserts with host_stage2_chunks == 0 holds only if the device's rules take every
    chunk libzstd level 1 and liblz4 write for these clouds: the restated rules decode each to the oracle's stage-1 payload,
    within the capacity of a slot. (A message that repeats an earlier one has its chunks checked once.)"""
    info, _ = S.cloud(family, 32768)
    capacity = oracle.stage1_bound(info, 32768) + 60
    for comp in S.COMPRESSIONS:
        msgs, sizes = S.directory(oracle, family, comp)
        assert sum(S.chunks_of_points(n) for n in sizes) == sum(len(p) for _m, p, _b in msgs) == 13
        seen = set()
        for _msg, payloads, body in msgs:
            blocks = lz4_body.chunks_of(body)
            assert len(blocks) == len(payloads)
            for blk, payload in zip(blocks, payloads):
                key = blk.tobytes()
                if key in seen:
                    continue
                seen.add(key)
                if comp == CompressionOption.LZ4:
                    assert LR.decode(key, capacity) == payload.tobytes()
                else:
                    verdict, got = ZR.decode(key, capacity)
                    assert verdict == ZR.OK and got == payload.tobytes()
        assert len(seen) >= 8
