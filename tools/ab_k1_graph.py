#!/usr/bin/env python3
"""A/B of K1 between builds of the library: per build one hipGraph of 500 launches (1M rows, 8 rotating buffers);
builds are interleaved, each measured as the mean of 4 timed replays after 2 untimed ones.  usage: ab_k1_graph.py a.so b.so ...
A build given as `path@nofuse` is captured with so3_capture_fusion(0) (the switch is process-wide PER LOADED FILE: to compare one
build with and without fusion, give it under two file names).  AB_EAGER=n adds, per round and build, the time per launch of n eager
launches over the same buffers (columns `name/eager`)."""
import ctypes, sys
import torch

P = ctypes.c_void_p
dev = torch.device("cuda:0")
n, NB, K = 1_000_000, 8, 500
x = [torch.randn(n, 9, device=dev) for _ in range(NB)]
r = [torch.empty(n, 9, device=dev) for _ in range(NB)]
graphs = {}
side = torch.cuda.Stream()
EAGER = int(__import__("os").environ.get("AB_EAGER", "0"))
for spec in sys.argv[1:]:
    path, _, mode = spec.partition("@")
    lib = ctypes.CDLL(path)
    if mode == "nofuse":
        lib.so3_capture_fusion(0)
    lib.so3_project_fwd_f32.restype = ctypes.c_int
    lib.so3_project_fwd_f32.argtypes = [P, P, P, ctypes.c_int64, P]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = P(side.cuda_stream)
            for i in range(K):
                assert lib.so3_project_fwd_f32(P(x[i % NB].data_ptr()), P(r[i % NB].data_ptr()), None, n, st) == 0
    graphs[spec.split("/")[-1]] = (g, lib)
torch.cuda.synchronize()
names = list(graphs)
for rnd in range(int(__import__("os").environ.get("AB_ROUNDS", "4"))):
    line = []
    order = names[rnd % len(names):] + names[:rnd % len(names)]          # the order rotates: no build always runs behind the same one
    for name in order:
        g, _ = graphs[name]
        with torch.cuda.stream(side):
            g.replay(); g.replay()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            for _ in range(4):
                g.replay()
            b.record(side)
        torch.cuda.synchronize()
        line.append((name, a.elapsed_time(b) * 1e3 / (4 * K)))
        if EAGER:
            lib = graphs[name][1]
            with torch.cuda.stream(side):
                st = P(side.cuda_stream)
                for i in range(NB):
                    lib.so3_project_fwd_f32(P(x[i].data_ptr()), P(r[i].data_ptr()), None, n, st)
                a.record(side)
                for i in range(EAGER):
                    lib.so3_project_fwd_f32(P(x[i % NB].data_ptr()), P(r[i % NB].data_ptr()), None, n, st)
                b.record(side)
            torch.cuda.synchronize()
            line.append((name + "/eager", a.elapsed_time(b) * 1e3 / EAGER))
    print("  ".join("%s %.2f" % (n_, v) for n_, v in sorted(line, key=lambda kv: (kv[0].endswith("/eager"), names.index(kv[0].split("/eager")[0])))), flush=True)
