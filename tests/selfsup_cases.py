"""Shared inputs and the dense fp64 oracle of the self-supervised loss tests
(test_selfsup_loss.py on CPU, test_gpu_selfsup.py on the GPU)."""

import functools

import torch


@functools.lru_cache(maxsize=None)
def make_case(B, N, M, T):
    """randn*3 first cloud; the second cloud is M noisy copies of its rows;
    T small random flows.  CPU fp32 tensors: pc1 (B,N,3), flows (T,B,N,3),
    pc2 (B,M,3).  Cached: callers must not modify them."""
    g = torch.Generator().manual_seed(1000 * N + M)
    pc1 = torch.randn(B, N, 3, generator=g) * 3
    src = torch.randint(0, N, (B, M), generator=g)
    pc2 = pc1.gather(1, src.unsqueeze(-1).expand(B, M, 3)) + 0.3 * torch.randn(B, M, 3, generator=g)
    flows = torch.stack([0.3 * torch.randn(B, N, 3, generator=g) for _ in range(T)])
    return pc1, flows, pc2


def knn_dense(pc, k):
    """(B,N,3) -> (B,N,k) int64 nearest neighbours (self included), brute
    force in fp64."""
    d = ((pc.double().unsqueeze(2) - pc.double().unsqueeze(1)) ** 2).sum(-1)
    return d.topk(min(k, pc.shape[1]), dim=-1, largest=False).indices


def dense_oracle(pc1, flows, pc2, idx):
    """The loss terms by their definitions, dense, in fp64.  The warped
    cloud is formed in the inputs' own precision (it is an input of the
    distance, w_t = pc1 + f_t), everything after it in fp64.

    Returns dict: d1 (T,B,N), i1, d2 (T,B,M), i2, chamfer (T,), smooth (T,).
    Non-finite distances never win; a row without a finite candidate has
    index -1, distance +INF and adds 0 to the mean.
    """
    inf = float("inf")
    w = (pc1.unsqueeze(0) + flows).double()
    d = ((w.unsqueeze(3) - pc2.double()[None, :, None]) ** 2).sum(-1)  # T,B,N,M
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, inf))
    (d1, i1), (d2, i2) = d.min(dim=3), d.min(dim=2)
    i1 = torch.where(torch.isfinite(d1), i1, torch.full_like(i1, -1))
    i2 = torch.where(torch.isfinite(d2), i2, torch.full_like(i2, -1))
    fin = lambda x: torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    chamfer = fin(d1).mean(dim=(1, 2)) + fin(d2).mean(dim=(1, 2))
    T, B, N, _ = flows.shape
    k = idx.shape[-1]
    f = flows.double()
    nb = f.gather(2, idx.reshape(1, B, N * k, 1).expand(T, B, N * k, 3)).view(T, B, N, k, 3)
    smooth = ((nb - f.unsqueeze(3)) ** 2).sum(-1).mean(dim=(1, 2, 3))
    return dict(d1=d1, i1=i1, d2=d2, i2=i2, chamfer=chamfer, smooth=smooth)


def descent_epe(device):
    """Free flow tensor fitted to a rigidly shifted, row-permuted copy of
    the cloud with the default loss: final mean end-point error."""
    from pvraft_amd.model.graph import Graph
    from pvraft_amd.utils import self_supervised_loss

    g = torch.Generator().manual_seed(7)
    pc1 = torch.randn(1, 256, 3, generator=g) * 3
    shift = torch.tensor([0.2, -0.1, 0.15])
    pc2 = (pc1 + shift)[:, torch.randperm(256, generator=g)]
    pc1, pc2, shift = pc1.to(device), pc2.to(device), shift.to(device)
    batch = {"sequence": [pc1, pc2]}
    graph = Graph.build(pc1, 9)
    flow = torch.zeros(1, 256, 3, device=device, requires_grad=True)
    opt = torch.optim.Adam([flow], lr=0.01)
    epe = lambda: (flow.detach() - shift).norm(dim=-1).mean().item()
    assert abs(epe() - 0.269) < 1e-3
    for _ in range(100):
        opt.zero_grad()
        self_supervised_loss(flow, batch, graph=graph).backward()
        opt.step()
    return epe()
