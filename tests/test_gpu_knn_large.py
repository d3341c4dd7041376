"""The knn edge style at the list sizes where the large kernel forms run.  tests/test_gpu_knn.py stops at about 120 atoms and
5 000 edges; here a batch has 1 053 .. 2 100 atoms, so that
  * knn_scan_kernel scans more than 1 024 atoms and more than 1 024 crystals (chunk > 1: the serial prefix inside a chunk, the two-level combine);
  * the Fourier operand of a build without a host round trip is the striding launch (capacity 96 N = 101 088 rows: more than 16 384 workgroups);
  * the two edge products run with a device-side row count on the forms gemm_planes chooses from a hint, also a hint far from the real count;
  * the backward pass sums in-edges over a list of 10 k edges and forms dZ2 as a plane set.
Inputs: tests/knn_cases.py (fixed seeds; no candidate pair within 1e-5 of a decision boundary, asserted before every bit comparison)."""
import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import knn_cases as K
from tests.gpu_util import load_decoder

pytestmark = pytest.mark.gpu

PLANES_DEFAULTS = (("mi_debug_set_planes_rt", (2, 16384)), ("mi_debug_set_planes_big", (1, 65536)), ("mi_debug_set_planes_dma", (1,)))
# the knob settings of the chain and forward tests: (label, setter, arguments)
FORMS = (("default", None, ()), ("rt(2, 1)", "mi_debug_set_planes_rt", (2, 1)), ("big(1, 8192)", "mi_debug_set_planes_big", (1, 8192)),
         ("dma(2)", "mi_debug_set_planes_dma", (2,)))


def _lib():
    from matinvent_amd import _lib as L
    return L, L.load()


def _restore_forms(lib):
    for name, args in PLANES_DEFAULTS:
        getattr(lib, name)(*args)


def _net(H, L, F, P=None):
    from matinvent_amd.cspnet import CSPNet
    net = CSPNet(hidden_dim=H, num_layers=L, num_freqs=F, latent_dim=256, ln=True, smooth=True, pred_type=True, edge_style="knn",
                 max_neighbors=K.MAX_NEIGHBORS, device="cuda")
    if P is not None:
        load_decoder(net, P)
    return net


def _assert_not_borderline(name):
    m = K.case_margin(name)
    assert m > K.MARGIN_MIN, f"{name}: a candidate pair sits {m:.2e} (relative) from a decision boundary -- choose another seed"


def _assert_list(edges, vec, edges_ref, vec_ref, what):
    assert edges.shape == edges_ref.shape, f"{what}: {edges.shape[1]} edges, the oracle has {edges_ref.shape[1]}"
    assert torch.equal(edges.cpu(), edges_ref), f"{what}: edge list differs from the oracle's"
    np.testing.assert_array_equal(vec.cpu().numpy(), vec_ref.numpy(), err_msg=what)   # exactly rounded: bit for bit


def _assert_csr(batch, edges_ref, vec_ref, what):
    """The source-sorted list the kernels iterate over is a permutation of the reference-order list."""
    ec, vc = batch.edges("csr")
    ec, vc = ec.cpu(), vc.cpu()
    assert ec.shape == edges_ref.shape, what
    assert bool((ec[0][1:] >= ec[0][:-1]).all()), f"{what}: CSR order must be sorted by source node"
    key = lambda e, v: sorted(zip(e[0].tolist(), e[1].tolist(), map(tuple, v.view(torch.int32).tolist())))   # (the vectors by their bits)
    assert key(ec, vc) == key(edges_ref, vec_ref), f"{what}: the CSR list is not a permutation of the reference-order list"


# ---- a. graph build --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A_dense", "B_dense", "B_sparse", "C_dense"])
def test_large_knn_graph_vs_oracle(name):
    """Edge list and edge vectors in the reference's order bit for bit, the CSR list a permutation of it sorted by source.  A: 1 053 atoms
    (scan chunk 2 over the atoms); B: 2 100 atoms in 1 050 crystals (chunk 3 / chunk 2), dense and from N(0,1) lattices with left-handed and
    near-singular cells and coordinates outside the home cell; C: two 64-atom crystals beside 1 100 single atoms (1 228 atoms, 1 102 crystals)."""
    _assert_not_borderline(name)
    frac, lat, na = K.inputs(name)
    edges_ref, vec_ref = K.reference(name)
    net = _net(64, 1, 4)
    b = net.make_batch(na.tolist())
    E = b.build_graph(frac, lat)
    print(f"{name}: {int(na.sum())} atoms, {len(na)} crystals, {E} edges (oracle {edges_ref.shape[1]}), margin {K.case_margin(name):.2e}")
    assert E == edges_ref.shape[1] == b.num_edges
    edges, vec = b.edges("reference")
    _assert_list(edges, vec, edges_ref, vec_ref, name)
    _assert_csr(b, edges_ref, vec_ref, name)


# ---- b. forward ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forward_case():
    """A dense at H = 256, L = 2, F = 32 with the float64 oracle's outputs (computed once)."""
    H, L, F = 256, 2, 32
    frac, lat, na = K.inputs("A_dense")
    B, N = len(na), int(na.sum())
    g = torch.Generator().manual_seed(5)
    at, t_emb = torch.randn(N, 100, generator=g), torch.randn(B, 256, generator=g)
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F, edge_style="knn")
    P = O.init_params(hp, seed=3)
    n2g = torch.repeat_interleave(torch.arange(B), na)
    edges, vec = K.reference("A_dense")
    d = lambda x: x.double()
    ref = O.cspnet_forward({k: d(v) for k, v in P.items()}, hp, d(t_emb), d(at), d(frac), d(lat), na, n2g, edges=edges, frac_diff=d(vec))
    return dict(H=H, L=L, F=F, P=P, at=at, t_emb=t_emb, ref=ref)


def test_large_knn_forward_vs_float64_oracle(forward_case):
    """Forward on A dense (21 912 edges) against the float64 oracle at the project's forward bound, 2e-5 of max(1, max|ref|), on every form
    the two edge products can take outside a chain (a synchronising build: the row count is the host's, M = E).  From gemm_planes, N = H = 256:
      product 1, FF [E, 192] x Wff^T -> M1 planes (row-major epilogue): the many-tile 128-row kernel (E < 65 536 rows; 2 x 176 workgroups > 256);
        gemm_planes_big_kernel under big(1, 8192); gemm_planes_dma_kernel under dma(2).  NOT gemm_rt, whatever rt(2, 1) says: its condition starts
        with `W.frag`, and net_forward hands make_planes(net->Wffpl ...) / make_planes(net->W2pl ...) without a fragment-order copy;
      product 2, M1 [E, 256] x W2^T with the segmented-sum epilogue (pe.seg_part: planes_epilogue_is_rows is false, so neither gemm_rt nor the big
        kernel): the many-tile 128-row kernel; gemm_planes_dma_kernel under dma(2).
    Measured on MI355X, error / max(1, max|ref|), the same under all four settings to the digits shown:
        pred_l 1.5e-07   pred_x 2.7e-07   pred_t 3.1e-07        (bound 2e-5)
    The float32 oracle's own error against float64 on this input: pred_l 3.8e-07, pred_x 5.0e-07, pred_t 6.6e-07 (max|ref| 12.8, 2.11, 2.47)."""
    _assert_not_borderline("A_dense")
    L_, lib = _lib()
    c = forward_case
    frac, lat, na = K.inputs("A_dense")
    net = _net(c["H"], c["L"], c["F"], c["P"])
    b = net.make_batch(na.tolist())
    try:
        for label, setter, args in FORMS:
            if setter:
                L_.check(getattr(lib, setter)(*args))
            try:
                with torch.no_grad():
                    out = net(c["t_emb"].cuda(), c["at"].cuda(), frac.cuda(), lat.cuda(), None, batch=b)
            finally:
                _restore_forms(lib)
            assert b._lib.mi_batch_num_edges(b._h) == K.reference("A_dense")[0].shape[1]
            errs = []
            for what, a, r in zip(("pred_l", "pred_x", "pred_t"), out, c["ref"]):
                scale = max(1.0, float(r.abs().max()))
                errs.append((what, float((a.double().cpu() - r).abs().max()) / scale))
            print(f"forward [{label}]: " + "  ".join(f"{w} {e:.2e}" for w, e in errs))
            for what, e in errs:
                assert e <= 2e-5, f"{what} [{label}]: {e:.3e} of max(1, max|ref|) > 2e-5"
    finally:
        _restore_forms(lib)


# ---- chains ----------------------------------------------------------------------------------------------------------------------
CHAIN_T, CHAIN_START, CHAIN_STOP = 50, 3, 0


@pytest.fixture(scope="module")
def chain_module():
    """H = 256, L = 2, F = 32, head weights scaled by 1e-2 (the cells stay well conditioned over the few steps), T = 50."""
    from matinvent_amd.diffcsp import DiffCSPModule
    hp = O.CSPNetHParams(hidden_dim=256, num_layers=2, num_freqs=32, edge_style="knn")
    P = O.init_params(hp, seed=1, head_scale=1e-2)
    m = DiffCSPModule(decoder=dict(hidden_dim=256, num_layers=2, num_freqs=32, ln=True, edge_style="knn", max_neighbors=K.MAX_NEIGHBORS),
                      beta_scheduler=dict(timesteps=CHAIN_T, scheduler_mode="cosine"),
                      sigma_scheduler=dict(timesteps=CHAIN_T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.ones(CHAIN_T + 1)), device="cuda")
    load_decoder(m.decoder, P)
    return m


def _init_state(name):
    frac, lat, na = K.inputs(name)
    a = torch.randn(int(na.sum()), 100, generator=torch.Generator().manual_seed(17))
    return frac, lat, a


def _chain(m, cb, name, seed=41):
    """A recorded chain of CHAIN_START steps from the named state on the handle `cb`; the steps' recorded tensors, in a fixed order."""
    _, traj = m.sample(cb, step_lr=5e-6, seed=seed, init=_init_state(name), t_start=CHAIN_START, t_stop=CHAIN_STOP, record=True)
    out = []
    for t in sorted(traj):
        for k in sorted(traj[t]):
            if k not in ("num_atoms", "batch_idx"):
                out.append(((t, k), traj[t][k].clone()))
    return out


def _assert_same_chain(a, b, what):
    assert [k for k, _ in a] == [k for k, _ in b], what
    for (k, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), (what, k, float((x - y).abs().max()))
    assert all(bool(torch.isfinite(x).all()) for _, x in a), what


def test_large_knn_chain_is_the_same_on_every_form_and_without_a_host_round_trip(chain_module):
    """A three-step chain from A dense (about 21.9 k edges, capacity 101 088 rows) under mi_debug_set_knn_nosync 0 / 1 / 2, each with the
    default thresholds, rt(2, 1), big(1, 8192) and dma(2): twelve recorded trajectories, all torch.equal (tests/test_gpu_gemm.py establishes
    that the forms agree bit for bit on a host-side row count).  Every chain runs on a fresh handle, so under mode 2 the hint is 0 and the forms
    are chosen for the CAPACITY; under mode 1 the first build tells the host the count; under mode 0 every build does and M = E.
    Forms, from gemm_planes (N = H = 256, two column tiles; Ms = the rows the form is chosen for):
      product 1 (FF x Wff^T, K = 192, row-major epilogue into the M1 planes):
        default     Ms = 21.9 k: the many-tile 128-row kernel (352 workgroups > 256: not the latency form);  mode 2: Ms = 101 088 >= 65 536:
                    gemm_planes_big_kernel with the device-side count
        rt(2, 1)    as default: gemm_rt cannot take a knn launch of the forward -- its condition in gemm_planes starts with `W.frag`, and
                    net_forward builds both weight operands with make_planes(...) alone, without the fragment-order copy
        big(1,8192) gemm_planes_big_kernel in every mode
        dma(2)      gemm_planes_dma_kernel (mode 2: the big kernel still comes first in the chain of conditions)
      product 2 (M1 x W2^T, K = 256, segmented-sum epilogue pe.seg_part, so planes_epilogue_is_rows is false: never gemm_rt or the big kernel):
        default / rt / big   the many-tile 128-row kernel with the segmented-sum epilogue;   dma(2)   gemm_planes_dma_kernel
    Under modes 1 and 2 the Fourier operand is the striding launch: 101 120 padded rows x 48 threads are 18 960 workgroups' worth, on 16 384."""
    L_, lib = _lib()
    m = chain_module
    _, _, na = K.inputs("A_dense")
    was = lib.mi_debug_set_knn_nosync(0)
    runs = []
    try:
        for mode in (0, 1, 2):
            for label, setter, args in FORMS:
                lib.mi_debug_set_knn_nosync(mode)
                if setter:
                    L_.check(getattr(lib, setter)(*args))
                try:
                    cb = m.make_batch(na.tolist())
                    runs.append((f"nosync {mode}, {label}", _chain(m, cb, "A_dense")))
                    m.check_graph()
                finally:
                    _restore_forms(lib)
    finally:
        lib.mi_debug_set_knn_nosync(was)
        _restore_forms(lib)
        m.__dict__["_knn_pending"] = []
    assert len(runs) == 12
    for what, r in runs[1:]:
        _assert_same_chain(runs[0][1], r, f"{what} against {runs[0][0]}")


@pytest.mark.parametrize("first,second", [("A_sparse", "A_dense"), ("A_dense", "A_sparse")])
def test_large_knn_chain_with_a_stale_hint_equals_the_chain_on_a_fresh_handle(chain_module, first, second):
    """One handle, no synchronising build at all (mode 2): a chain from `first`, then a chain from `second`.  The second chain's launches are
    shaped by what the first left behind -- the hint of its last list (sparse: 4.7 k edges, dense: 21.9 k) and its tables -- and must still be
    bit for bit the chain on a fresh handle whose every build synchronises (mode 0).  Sparse -> dense: product 2 is chosen for 4.7 k rows (80
    workgroups <= 256: gemm_planes_dma_kernel under the default dma(1)) and meets 21.9 k; dense -> sparse: the many-tile kernels meet 4.7 k rows,
    most tiles past the count."""
    L_, lib = _lib()
    m = chain_module
    _, _, na = K.inputs(second)
    was = lib.mi_debug_set_knn_nosync(0)
    try:
        want = _chain(m, m.make_batch(na.tolist()), second)
        m.check_graph()
        lib.mi_debug_set_knn_nosync(2)
        cb = m.make_batch(na.tolist())
        _chain(m, cb, first)
        got = _chain(m, cb, second)     # (sample() reads the first chain's verdict and count first: the stale hint)
        m.check_graph()
    finally:
        lib.mi_debug_set_knn_nosync(was)
        m.__dict__["_knn_pending"] = []
    _assert_same_chain(want, got, f"{second} behind {first} on one handle")


# ---- f. handle state -------------------------------------------------------------------------------------------------------------
def test_large_knn_handle_describes_the_last_list_after_a_chain_without_a_host_round_trip(chain_module):
    """After a chain whose builds never synchronised and check_graph(), the handle reports the chain's last list: its true edge count -- not
    the capacity the launches were sized for -- and exactly the rows the same chain leaves when every build synchronises."""
    L_, lib = _lib()
    m = chain_module
    _, _, na = K.inputs("A_dense")
    N = int(na.sum())
    was = lib.mi_debug_set_knn_nosync(0)
    try:
        cb0 = m.make_batch(na.tolist())
        _chain(m, cb0, "A_dense")
        m.check_graph()
        lib.mi_debug_set_knn_nosync(2)
        cb2 = m.make_batch(na.tolist())
        _chain(m, cb2, "A_dense")
        assert int(lib.mi_batch_num_edges(cb2._h)) == 96 * N   # (the chain did run without a round trip: until the verdict is read, the capacity)
        m.check_graph()
    finally:
        lib.mi_debug_set_knn_nosync(was)
        m.__dict__["_knn_pending"] = []
    E0 = int(lib.mi_batch_num_edges(cb0._h))
    E2 = int(lib.mi_batch_num_edges(cb2._h))
    print(f"edges of the chain's last list: {E0} (synchronising), {E2} (no round trip); capacity {96 * N}")
    assert 0 < E0 < 96 * N and E0 % 2 == 0
    assert E2 == E0 and cb2.num_edges == E0 and cb0.num_edges == E0
    (e0, v0), (e2, v2) = cb0.edges("reference"), cb2.edges("reference")
    assert e2.shape == (2, E0) and v2.shape == (E0, 3)
    assert torch.equal(e0, e2) and torch.equal(v0, v2)
    (c0, w0), (c2, w2) = cb0.edges("csr"), cb2.edges("csr")
    assert torch.equal(c0, c2) and torch.equal(w0, w2)
    _assert_csr(cb2, e2.cpu(), v2.cpu(), "the list behind the chain")
    assert int(e2.min()) >= 0 and int(e2.max()) < N


# ---- e. gradients ----------------------------------------------------------------------------------------------------------------
def test_large_knn_grads_vs_float64_oracle():
    """dLoss/dtheta through a knn list of 10 228 edges (501 atoms; H = 128, L = 2, F = 16) against float64 oracle autograd, per tensor at the
    fully connected tests' bound: 2e-5 of max|grad|.  Above 8 192 edges the backward forms dZ2 as a plane set; the in-edge sums run over
    `inedge` spans of up to 29 edges.  tests/test_gpu_knn.py holds the same quantities at 38 atoms to 5e-4.
    Measured on MI355X (the test prints every tensor): worst 7.2e-07 of max|grad| (csp_layer_1.edge_mlp.0.bias), every tensor between 1.0e-07
    and 7.2e-07; the forward outputs 2.3e-07 / 5.0e-07 / 4.1e-07 of max(1, max|ref|).  The knn backward meets the fully connected bound with a
    factor of 28 to spare: the 5e-4 of the small test is not a property of the kernels (its reference is float32 autograd)."""
    _assert_not_borderline("G_dense")
    H, L, F = 128, 2, 16
    frac, lat, na = K.inputs("G_dense")
    edges, vec = K.reference("G_dense")
    B, N = len(na), int(na.sum())
    g = torch.Generator().manual_seed(5)
    at, t_emb = torch.randn(N, 100, generator=g), torch.randn(B, 256, generator=g)
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F, edge_style="knn")
    P = O.init_params(hp, seed=3)
    d = lambda x: x.double()
    Pg = {k: d(v).requires_grad_(True) for k, v in P.items()}
    n2g = torch.repeat_interleave(torch.arange(B), na)
    pl, px, pt = O.cspnet_forward(Pg, hp, d(t_emb), d(at), d(frac), d(lat), na, n2g, edges=edges, frac_diff=d(vec))
    wl, wx, wt = (torch.randn(p.shape, generator=g) for p in (pl, px, pt))
    ((pl * d(wl)).sum() + (px * d(wx)).sum() + (pt * d(wt)).sum()).backward()

    net = _net(H, L, F, P)
    net.theta.requires_grad_(True)
    b = net.make_batch(na.tolist())
    with torch.enable_grad():
        ql, qx, qt = net(t_emb.cuda(), at.cuda(), frac.cuda(), lat.cuda(), None, batch=b)
        (ql * wl.cuda()).sum().add((qx * wx.cuda()).sum()).add((qt * wt.cuda()).sum()).backward()
    assert b._lib.mi_batch_num_edges(b._h) == edges.shape[1] > 8192
    for what, a, r in (("pred_l", ql, pl), ("pred_x", qx, px), ("pred_t", qt, pt)):
        r = r.detach()
        e = float((a.detach().double().cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"forward {what}: {e:.2e} of max(1, max|ref|)")
        assert e <= 2e-5, (what, e)
    rows = []
    for k, (o, n, shape) in net.layout.items():
        ref = Pg["decoder." + k].grad
        got = net.theta.grad[o:o + n].view(shape).double().cpu()
        scale = float(ref.abs().max())
        rows.append((float((got - ref).abs().max()) / scale, k, scale))
    for e, k, scale in sorted(rows, reverse=True):
        print(f"grad {k}: {e:.2e} of max|grad| = {scale:.3e}")
    worst = max(rows)
    assert worst[0] <= 2e-5, f"grad {worst[1]}: {worst[0]:.3e} of max|grad| > 2e-5"
