"""CPU checks of what the large knn tests stand on: the seeds of tests/knn_cases.py keep every candidate pair away from the decision
boundaries of the neighbour search, and the oracle's forward follows the dtype of its arguments while the knn list stays float32's."""
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import knn_cases as K


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_no_candidate_pair_is_borderline(name):
    assert K.case_margin(name) > K.MARGIN_MIN


def test_margin_sees_a_pair_on_the_cutoff():
    """A cubic cell of edge a with one atom: the six nearest self images sit at d = a, the cutoff at a + 0.01 -- a relative distance of
    about 2 * 0.01 / a in d^2; moving the cutoff onto them (a second atom is not needed) must show as a small margin."""
    lat = 5.0 * torch.eye(3)[None]
    m = K.margin(torch.zeros(1, 3), lat, [1])
    assert abs(m - (1 - 25.0 / 5.01 ** 2)) < 1e-12
    # two atoms 1e-2 A apart along x: d^2 = 1e-4 is the self-pair floor itself
    m = K.margin(torch.tensor([[0.0, 0.0, 0.0], [0.002, 0.0, 0.0]]), lat, [2])
    assert m < 1e-6


def test_sparse_cases_hold_left_handed_and_near_singular_cells():
    for name in ("A_sparse", "B_sparse"):
        frac, lat, _ = K.inputs(name)
        det = torch.det(lat)
        assert bool((det < 0).any()) and bool((det > 0).any())
        assert float(det.abs().min()) < 1e-2
        assert float(frac.min()) < 0 and float(frac.max()) > 1


def test_oracle_forward_follows_the_dtype_and_keeps_the_float32_list():
    H, L, F = 32, 2, 4
    na = torch.tensor([6, 1, 11])
    frac, lat = K.dense(na.tolist(), 7)
    B, N = len(na), int(na.sum())
    g = torch.Generator().manual_seed(5)
    at, t_emb = torch.randn(N, 100, generator=g), torch.randn(B, 256, generator=g)
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F, edge_style="knn")
    P = O.init_params(hp, seed=3)
    n2g = torch.repeat_interleave(torch.arange(B), na)
    o32 = O.cspnet_forward(P, hp, t_emb, at, frac, lat, na, n2g)
    assert all(o.dtype == torch.float32 for o in o32)
    d = lambda x: x.double()
    P64 = {k: d(v).requires_grad_(True) for k, v in P.items()}
    taps = {}
    o64 = O.cspnet_forward(P64, hp, d(t_emb), d(at), d(frac), d(lat), na, n2g, taps=taps)
    assert all(o.dtype == torch.float64 for o in o64) and taps["ff"].dtype == torch.float64
    # the same list: the Fourier operand has one row per edge of the float32 list, and is the float64 sine / cosine of ITS float32 attribute
    edges, vec = O.knn_edges(frac, lat, na, hp.max_neighbors)
    assert taps["ff"].shape == (edges.shape[1], 6 * F)
    assert torch.equal(taps["ff"], O.sinusoids_embedding(d(vec), F))
    for a, b in zip(o32, o64):
        assert float((d(a) - b.detach()).abs().max()) <= 1e-5 * max(1.0, float(b.detach().abs().max()))
    sum(o.sum() for o in o64).backward()
    assert all(v.grad is not None and v.grad.dtype == torch.float64 for v in P64.values())
