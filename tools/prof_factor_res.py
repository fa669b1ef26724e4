#!/usr/bin/env python3
"""Time pq_factor_batched's inverse mode on COUNT identical SPD problems of size N and, with the
PQ_PROFILE library (PQ_LIB_PATH=porqua_amd/libporqua_hip_prof.so), print the resident kernel's phase
clocks (load / potrf / trtri / lauum / store per workgroup).  The route is the library's own choice
unless PQ_FACTOR_RES / PQ_FACTOR_SK force it -- experiment tooling, not a test.

    python tools/prof_factor_res.py [COUNT=250] [N=284]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from porqua_amd import _lib, engine  # noqa: E402


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 250
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 284
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(0)
    M = rng.standard_normal((n + 7, n))
    P1 = M.T @ M / n + 0.1 * np.eye(n)
    qb = engine.QPBatch.from_dense(np.broadcast_to(P1, (count, n, n)).copy(), np.zeros((count, n)), device=dev)
    s = engine.Settings(sigma=0.0).to_c()
    ws = engine.Workspace(qb)
    pb = qb.c_struct()
    pb.mg = 0
    pb.lb = pb.ub = None
    st = ws.c_struct()
    strm = engine._stream()
    _lib.check(lib.pq_init_state(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s), strm), "init")

    def run():
        _lib.check(lib.pq_factor_batched(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s), 2, strm),
                   "pq_factor_batched")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    lib.pq_factor_last_route.restype = ctypes.c_int
    route = int(lib.pq_factor_last_route())
    ref = np.linalg.inv(P1)
    err = np.abs(ws.K[0, :n, :n].cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"count={count} n={n} ld={qb.ld} route={route} (0 k_factor, 1 k_factor_sk, 2 k_factor_res) "
          f"us median={np.median(ts):.1f} min={min(ts):.1f} relerr={err:.2e}")
    if route == 2:
        nb = min(count, 1024)
        buf = (ctypes.c_longlong * (8 * nb))()
        lib.pq_factor_res_prof.restype = ctypes.c_int
        if lib.pq_factor_res_prof(buf, ctypes.c_int32(nb)) == 0:
            a = np.array(buf[:], dtype=np.float64).reshape(nb, 8)[:, :5] * 10e-3   # 100 MHz ticks -> us
            print("phase us (load potrf trtri lauum store): median", np.round(np.median(a, 0), 1),
                  "max", np.round(a.max(0), 1), "sum-median", round(float(np.median(a.sum(1))), 1))
        else:
            print("(no phase clocks: not a PQ_PROFILE build)")


if __name__ == "__main__":
    main()
