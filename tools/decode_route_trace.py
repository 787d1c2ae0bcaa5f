#!/usr/bin/env python3
"""The decode routes on the GPU, against the table of tests/test_decode_route.py.

    rocprofv3 --kernel-trace -d DIR -o trace -- python tools/decode_route_trace.py run
    python tools/decode_route_trace.py names DIR/.../trace_results.db > branch.txt
    python tools/decode_route_trace.py expect > expect.txt          # decode_route_kernels() of every traced row (CPU only)
    python tools/decode_route_trace.py design                       # the route table of DESIGN.md section 4 (CPU only)

`run` decodes one small device-resident batch per row of the table that the C ABI can produce (2 chunks: 32768 + 100 points;
the rows that say so 65 chunks, or with the launch hints primed by earlier calls) through cldn_hip_decode_stage1_sized /
cldn_hip_decode_lz4 and prints the row names. A marker kernel of torch in front of and behind the traced call separates the
rows in the trace; `names` prints `row: kernels in launch order` from it. Two libraries (CLDN_HIP_LIB_OVERRIDE) traced this
way must give the same lines, and both the lines of `expect`."""
import importlib.util
import os
import re
import sqlite3
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("test_decode_route", os.path.join(ROOT, "tests", "test_decode_route.py"))
table = importlib.util.module_from_spec(spec)
spec.loader.exec_module(table)
ROWS = [r for r in table.ROWS if r["call"].get("gpu", 1)]
NP_TYPES = {4: "<u2", 6: "<u4", 7: "<f4", 8: "<f8", 10: "<u8"}


def make_cloud(r, n):
    """(EncodingInfo, bytes of n points) of the row's schema: floats walk, the integer fields as the row's `data` says."""
    import numpy as np
    from cloudini_amd.schema import CompressionOption, EncodingInfo, EncodingOptions, FieldType, PointField
    rs = np.random.RandomState(7)
    step = r["step"]
    fields = [PointField(f"f{i}", off, FieldType(t), 0.001 if res else None) for i, (t, off, res) in enumerate(r["fields"])]
    info = EncodingInfo(fields=fields, width=n, height=1, point_step=step, compression_opt=CompressionOption.NONE,
                        encoding_opt=EncodingOptions.LOSSLESS if r["call"].get("lossless") else EncodingOptions.LOSSY)
    data = np.zeros((n, step), dtype=np.uint8)
    kind = r["call"].get("data", "walk")
    for t, off, _res in r["fields"]:
        dt = np.dtype(NP_TYPES[t])
        if dt.kind == "f":
            v = np.cumsum(rs.uniform(-0.01, 0.01, n)).astype(dt)
        elif kind == "few":
            v = rs.randint(0, 6, n).astype(dt)
        elif kind == "runs":
            v = (np.arange(n) // 64).astype(dt)
        else:
            v = (1000 + np.cumsum(rs.randint(-3, 4, n))).astype(dt)
        data[:, off:off + dt.itemsize] = v.view(np.uint8).reshape(n, dt.itemsize)
    return info, data.reshape(-1)


def run():
    import numpy as np
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    sep = torch.zeros(64, dtype=torch.float64, device=dev)  # its cos_() is the marker kernel
    for r in ROWS:
        c = r["call"]
        n = (c.get("n_chunks", 2) - 1) * 32768 + 100
        info, host = make_cloud(r, n)
        plan = native.Plan(info)
        codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        if c.get("fill_zero"):
            codec.set_decode_fill(True)
        if c.get("lz4"):
            codec.set_stage2(1)
        if c.get("force_parts"):
            assert codec.decode_split(c["force_parts"]) == 0
        cp = np.array([n], dtype=np.uint64)
        cap = plan.stage2_bound(n, 1 if c.get("lz4") else 0)
        d_points = torch.from_numpy(host).to(dev)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.empty(2, dtype=torch.int64, device=dev)
        d_sizes = torch.empty(c.get("n_chunks", 2), dtype=torch.int32, device=dev)
        codec.encode_device(d_points.data_ptr(), cp, d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
        torch.cuda.synchronize()
        offs = d_off.cpu().numpy().astype(np.uint64)
        d_dec = torch.empty(host.size + 64, dtype=torch.uint8, device=dev)
        out_ptr = d_dec.data_ptr() + (0 if c.get("aligned", 1) else 4)

        def decode():
            if c.get("lz4"):
                codec.decode_lz4_device(d_out.data_ptr(), offs, cp, out_ptr, host.size)
            else:
                codec.decode_device(d_out.data_ptr(), offs, cp, out_ptr, host.size, d_sizes.data_ptr() if c.get("sized", 1) else 0)
            torch.cuda.synchronize()

        for _ in range(3 if ("palette_hint" in c or "dv_hint" in c) else 0):  # the hints follow the counters of earlier calls
            decode()
        sep.cos_()
        decode()
        sep.cos_()
        torch.cuda.synchronize()
        codec.status()
        print(r["name"], flush=True)
        codec.close()


def names(db):
    con = sqlite3.connect(db)
    cur = con.execute("select * from kernels limit 0")
    cols = [d[0] for d in cur.description]
    order = "start" if "start" in cols else "rowid"
    rows, inside, mine = [], False, []
    for (name,) in con.execute(f"select name from kernels order by {order}"):
        if "cldn" not in name:
            if "cos" in name:
                if inside:
                    rows.append(mine)
                inside, mine = not inside, []
            continue
        m = re.search(r"\b(k_[a-z0-9_]+)", name)
        if inside and m:
            mine.append(m.group(1))
    assert len(rows) == len(ROWS), (len(rows), len(ROWS))
    for r, ks in zip(ROWS, rows):
        print(f"{r['name']}: {' '.join(ks)}")


def expect():
    L = table.build_shim(tempfile.mkdtemp())
    for r in ROWS:
        print(f"{r['name']}: {' '.join(table.route_of(L, r)[0])}")


def design():
    print("\n".join(table.design_table(table.build_shim(tempfile.mkdtemp()))))


if __name__ == "__main__":
    {"run": run, "names": lambda: names(sys.argv[2]), "expect": expect, "design": design}[sys.argv[1]]()
