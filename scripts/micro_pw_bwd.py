"""Microbenchmark: the fused conv-stack data gradient (_C.pw_bwd) against
the composed path it replaces (threshold_backward + transpose + one bmm per
part), on the flagship shapes (B=2, S=8192, bf16).

Each variant is captured into a hipGraph of REPS calls (so the figure is
device time, not Python launch time), and the two graphs are replayed
alternately in ~50 ms blocks between device events; the per-call time is
the median over blocks.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import pvraft_amd._C as C

B, S = 2, 8192
REPS = 20
BLOCK_MS = 50.0
BLOCKS = 8

# (name, Co, [(Ci, wanted)], relu, point_major, slab)
SHAPES = [
    ("conv_corr/fc2/knn_out", 64, [(64, True)], False, False, False),
    ("motion", 61, [(64, True), (64, True)], True, False, False),
    ("gates m", 192, [(61, True), (3, False)], False, False, False),
    ("gates zr (slab)", 128, [(64, True)], False, False, True),
    ("gates q (slab)", 64, [(64, True)], False, False, True),
    ("out_conv[0]", 64, [(64, True), (64, True)], True, False, False),
    ("SetConv fc1 (point-major)", 64, [(64, True), (3, False)], False, True, False),
    ("corr MLP", 128, [(81, True)], False, False, False),
]


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


def ab(fa, fb):
    """median us per call of fa and fb, alternated in ~50 ms blocks"""
    ga, gb = graph_of(fa), graph_of(fb)
    out = []
    reps = {}
    for g in (ga, gb):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        reps[g] = max(1, int(BLOCK_MS / (e0.elapsed_time(e1) / 10)))
    ts = {ga: [], gb: []}
    for _ in range(BLOCKS):
        for g in (ga, gb):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(reps[g]):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts[g].append(e0.elapsed_time(e1) * 1e3 / (reps[g] * REPS))
    for g in (ga, gb):
        v = sorted(ts[g])
        out.append((v[len(v) // 2], v[0], v[-1]))
    return out


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"pw_bwd vs composed, B={B} S={S} bf16: median us/call (min..max over blocks)")
    for name, Co, parts, relu, pm, slab in SHAPES:
        shape = (B, S, Co) if pm else (B, Co, S)
        dy = torch.randn(shape, device=dev).bfloat16()
        y = torch.randn(shape, device=dev).relu().bfloat16()
        ws = [(torch.randn(Co, ci, device=dev) * 0.1).bfloat16() for ci, _ in parts]
        want = [k for _, k in parts]
        act = 1 if relu else 0
        buf = torch.empty(B, 192, S, device=dev, dtype=torch.bfloat16) if slab else None

        def fused():
            return C.pw_bwd(dy, y if relu else None, ws, want, act, pm, buf, 0)

        def composed():
            d = torch.ops.aten.threshold_backward(dy, y, 0) if relu else dy
            if pm:
                d = C.batched_transpose(d)
            outs = [torch.bmm(w.t().unsqueeze(0).expand(B, -1, -1), d)
                    for w, k in zip(ws, want) if k]
            if slab:
                # autograd's slice gradient: zero-filled full tensor + copy
                full = torch.zeros(B, 192, S, device=dev, dtype=torch.bfloat16)
                full[:, :Co] = d
                outs.append(full)
            return outs

        (fm, f0, f1), (cm, c0, c1) = ab(fused, composed)
        print(f"{name:28s} Co={Co:3d} Ci={'+'.join(str(c) for c, _ in parts):7s} "
              f"pw_bwd {fm:6.2f} ({f0:.2f}..{f1:.2f})  "
              f"composed {cm:6.2f} ({c0:.2f}..{c1:.2f})  x{cm / fm:.2f}")

    # pw_fwd: pw_stage.h staging against PVRAFT_PW_STAGE=classic.  The
    # launcher reads the variable per launch, so each captured graph keeps
    # the kernel it was captured with.
    print("pw_fwd new vs classic staging: median us/call (min..max over blocks)")
    for name, Co, parts, relu, pm, _slab in SHAPES:
        ws = [(torch.randn(Co, ci, device=dev) * 0.1).bfloat16() for ci, _ in parts]
        xs = [torch.randn(B, ci, S, device=dev).bfloat16() for ci, _ in parts]
        bias = torch.randn(Co, device=dev)
        act = 1 if relu else 0

        def fwd_new():
            os.environ.pop("PVRAFT_PW_STAGE", None)
            return C.pw_fwd(ws, xs, bias, None, act, pm)

        def fwd_classic():
            os.environ["PVRAFT_PW_STAGE"] = "classic"
            y = C.pw_fwd(ws, xs, bias, None, act, pm)
            os.environ.pop("PVRAFT_PW_STAGE", None)
            return y

        (nm, n0, n1), (cm, c0, c1) = ab(fwd_new, fwd_classic)
        print(f"{name:28s} Co={Co:3d} Ci={'+'.join(str(c) for c, _ in parts):7s} "
              f"new {nm:6.2f} ({n0:.2f}..{n1:.2f})  "
              f"classic {cm:6.2f} ({c0:.2f}..{c1:.2f})  x{cm / nm:.2f}")


if __name__ == "__main__":
    main()
