"""GPU tests of the counting-sort inverse adjacency (csrc/knn_csr.hip)
against the stable-argsort torch composition.  Run with -m gpu."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def csr_oracle(idx32):
    """Graph.csr()'s torch composition with the argsort made stable."""
    B, N, k = idx32.shape
    flat = idx32.long().permute(0, 2, 1).reshape(B, k * N)
    order = flat.argsort(dim=1, stable=True)
    targets = flat.gather(1, order)
    bounds = torch.arange(N + 1, device=flat.device).expand(B, N + 1).contiguous()
    offsets = torch.searchsorted(targets, bounds, side="left")
    return (
        order.to(torch.int32),
        offsets.to(torch.int32),
        (order % N).to(torch.int32),
        (order // N).to(torch.uint8),
    )


def knn_idx32(B, N, k, seed=0):
    from pvraft_amd import _C

    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, 3, generator=g).to(dev())
    return _C.knn_graph(xyz.contiguous(), k)


def check_equal(idx32):
    from pvraft_amd import _C

    B, N, k = idx32.shape
    got = _C.knn_csr(idx32)
    want = csr_oracle(idx32)
    assert got[0].shape == (B, k * N) and got[1].shape == (B, N + 1)
    assert got[2].shape == (B, k * N) and got[3].shape == (B, k * N)
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.int32, torch.uint8]
    for name, g, w in zip(("order", "offsets", "order_n", "order_j"), got, want):
        assert torch.equal(g, w), name
    assert bool((got[1][:, N] == k * N).all())


@pytest.mark.parametrize(
    "B,N,k", [(2, 500, 16), (1, 127, 8), (3, 64, 48), (1, 8192, 32)]
)
def test_knn_graph_cases_match_stable_argsort(B, N, k):
    check_equal(knn_idx32(B, N, k))


def test_hub_node_and_empty_rows():
    B, N, k = 2, 300, 4
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(1, 10, (B, N, k), generator=g, dtype=torch.int32)
    idx[:, :, 0] = 0  # node 0: in-degree N; nodes >= 10: in-degree 0
    check_equal(idx.to(dev()).contiguous())


def test_rows_repeating_one_value():
    B, N, k = 2, 200, 8
    g = torch.Generator().manual_seed(2)
    per_row = torch.randint(0, N, (B, N, 1), generator=g, dtype=torch.int32)
    check_equal(per_row.expand(B, N, k).contiguous().to(dev()))


def test_two_calls_are_bit_equal():
    from pvraft_amd import _C

    idx32 = knn_idx32(2, 500, 16)
    a = _C.knn_csr(idx32)
    b = _C.knn_csr(idx32)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_graph_replay_follows_the_static_buffer():
    from pvraft_amd import _C

    first = knn_idx32(2, 500, 16, seed=3)
    second = knn_idx32(2, 500, 16, seed=4)
    assert not torch.equal(first, second)
    want = [t.clone() for t in _C.knn_csr(second)]
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _C.knn_csr(static)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _C.knn_csr(static)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(out, want):
        assert torch.equal(g, w)


def test_graph_csr_uses_the_op_and_matches_torch_toggle(monkeypatch):
    from pvraft_amd.model.graph import Graph

    g = torch.Generator().manual_seed(5)
    xyz = torch.randn(2, 500, 3, generator=g).to(dev())
    graph = Graph.build(xyz, 16)
    assert graph._idx32 is not None and graph._idx32.dtype == torch.int32
    assert torch.equal(graph.idx, graph._idx32.long())
    got = graph.csr()
    want = csr_oracle(graph.idx32)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    monkeypatch.setenv("PVRAFT_CSR", "torch")
    fallback = Graph(idx=graph.idx, xyz=xyz).csr()
    assert fallback[1].dtype == torch.int32 and torch.equal(fallback[1], want[1])
