"""Microbenchmark: the pieces of the truncated-correlation backward and of
the forward's candidate gather at the flagship shape (B=2, N=M=8192, K=512,
C=128, bf16): corr_grad_expand against zeros + mul + cast + scatter_, the
three ways to feed the g1 GEMM, the g2 GEMM, corr_gather_xyz against
long() + ATen gather.

Each variant is captured into a hipGraph of REPS calls (device time, not
Python launch time); the graphs are replayed in turn in ~50 ms blocks
between device events and the per-call time is the median over blocks.
"""

import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import pvraft_amd._C as C

B, N, M, K, CH = 2, 8192, 8192, 512, 128
REPS = 10
BLOCK_MS = 50.0
BLOCKS = 6


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def timed(fns):
    """{name: (median, min, max) us per call}, variants alternated"""
    graphs = {k: graph_of(f) for k, f in fns.items()}
    reps = {}
    for k, g in graphs.items():
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(5):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        reps[k] = max(1, int(BLOCK_MS / (e0.elapsed_time(e1) / 5)))
    ts = {k: [] for k in graphs}
    for _ in range(BLOCKS):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(reps[k]):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / (reps[k] * REPS))
    out = {}
    for k, v in ts.items():
        v = sorted(v)
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def show(title, res):
    print(title)
    for k, (m, lo, hi) in res.items():
        print(f"  {k:44s} {m:8.2f} us ({lo:.2f}..{hi:.2f})")


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    scale = 1.0 / math.sqrt(CH)
    idx32 = torch.rand(B, N, M, device=dev).topk(K, dim=2).indices.to(torch.int32)
    idx64 = idx32.long()
    g = torch.randn(B, N, K, device=dev)
    f1 = torch.randn(B, CH, N, device=dev).bfloat16()
    f2 = torch.randn(B, CH, M, device=dev).bfloat16()
    f2t = C.batched_transpose(f2)
    xyz2 = torch.randn(B, M, 3, device=dev)
    gfull = C.corr_grad_expand(g, idx32, scale, M, True)

    def expand_classic():
        full = torch.zeros(B, N, M, dtype=torch.bfloat16, device=dev)
        return full.scatter_(2, idx64, (g * scale).to(torch.bfloat16))

    assert torch.equal(gfull, expand_classic())
    show(f"dense gradient (B,N,M,K)=({B},{N},{M},{K}) bf16", timed({
        "corr_grad_expand": lambda: C.corr_grad_expand(g, idx32, scale, M, True),
        "zeros + mul + cast + scatter_": expand_classic,
        "torch.zeros alone": lambda: torch.zeros(B, N, M, dtype=torch.bfloat16, device=dev),
    }))

    show("g1 = f2 @ gfull^T, (B,C,N)", timed({
        "batched_transpose(gfull) + bmm(f2, gfull_t)":
            lambda: torch.bmm(f2, C.batched_transpose(gfull)),
        "bmm(f2, gfull_t) alone":
            (lambda t: (lambda: torch.bmm(f2, t)))(C.batched_transpose(gfull)),
        "bmm(f2, gfull.transpose(1, 2))":
            lambda: torch.bmm(f2, gfull.transpose(1, 2)),
        "bmm(gfull, f2t) + batched_transpose":
            lambda: C.batched_transpose(torch.bmm(gfull, f2t)),
        "g2 = bmm(f1, gfull)": lambda: torch.bmm(f1, gfull),
    }))

    def gather_classic():
        i = idx32.long()
        return xyz2.gather(
            1, i.reshape(B, N * K).unsqueeze(-1).expand(B, N * K, 3)
        ).view(B, N, K, 3)

    assert torch.equal(C.corr_gather_xyz(idx32, xyz2), gather_classic())
    show("txyz = xyz2 rows at idx", timed({
        "corr_gather_xyz": lambda: C.corr_gather_xyz(idx32, xyz2),
        "idx.long() + ATen gather": gather_classic,
    }))


if __name__ == "__main__":
    main()
