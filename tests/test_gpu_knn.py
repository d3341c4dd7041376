"""GPU parity of the periodic neighbour graph (K17) and of the score network on top of it:
CSPNet.gen_edges knn branch = radius_graph_pbc + get_max_neighbors_mask + reorder_symmetric_edges
(models/diffcsp/cspnet.py:159-257, models/diffcsp/utils.py:335-601).  The edge list and its attribute are index /
exactly-rounded work: compared bit for bit, in the reference's order.  Network outputs: fp32 round-off."""
import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests.gpu_util import load_decoder, params_from_golden

pytestmark = pytest.mark.gpu


def _net(H, L, F, P=None, seed=0):
    from matinvent_amd.cspnet import CSPNet
    torch.manual_seed(seed)
    net = CSPNet(hidden_dim=H, num_layers=L, num_freqs=F, latent_dim=256, ln=True, smooth=True, pred_type=True, edge_style="knn",
                 max_neighbors=20, device="cuda")
    if P is not None:
        load_decoder(net, P)
    return net


def _close(a, b, tol, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.1e} * {scale:.3g}"


def _check_csr(batch, edges_ref, vec_ref, N):
    """The source-sorted list the kernels iterate over is a permutation of the reference list."""
    ec, vc = batch.edges("csr")
    ec, vc = ec.cpu(), vc.cpu()
    assert bool((ec[0][1:] >= ec[0][:-1]).all()), "CSR order must be sorted by source node"
    key = lambda e, v: sorted(zip(e[0].tolist(), e[1].tolist(), map(tuple, v.tolist())))
    assert key(ec, vc) == key(edges_ref, vec_ref)


def test_knn_graph_golden(golden):
    g = golden("g5c_knn")
    net = _net(64, 2, 8)
    b = net.make_batch(g["num_atoms"])
    E = b.build_graph(torch.from_numpy(g["frac"]), torch.from_numpy(g["lattices"]))
    assert E == g["edges"].shape[1]
    edges, vec = b.edges("reference")
    assert edges.cpu().tolist() == g["edges"].tolist()
    np.testing.assert_array_equal(vec.cpu().numpy(), g["edge_vec"])  # exactly rounded: bit for bit
    _check_csr(b, torch.from_numpy(g["edges"]), torch.from_numpy(g["edge_vec"]), int(g["num_atoms"].sum()))


def test_knn_forward_golden(golden):
    g = golden("g5c_knn")
    net = _net(64, 2, 8, params_from_golden(g))
    T = lambda k: torch.from_numpy(g[k]).cuda()
    b = net.make_batch(g["num_atoms"])
    for mode, edge in (("split", "gemm"), ("f32", "gemm"), ("f32", "fused_f32")):
        from matinvent_amd.cspnet import set_gemm_mode
        set_gemm_mode(mode)
        net.set_edge_mode(edge)
        try:
            pl, px, pt = net(T("t_emb"), T("atom_types"), T("frac"), T("lattices"), None, batch=b)
        finally:
            set_gemm_mode("split")
        assert b._lib.mi_batch_num_edges(b._h) == g["edges"].shape[1]
        _close(pl, g["pred_l"], 2e-5, f"pred_l [{mode}-{edge}]")
        _close(px, g["pred_x"], 2e-5, f"pred_x [{mode}-{edge}]")
        _close(pt, g["pred_t"], 2e-5, f"pred_t [{mode}-{edge}]")


def _random_crystals(seed, num_atoms, lo=3.5, hi=9.0, ang=(65.0, 115.0)):
    g = torch.Generator().manual_seed(seed)
    B, N = len(num_atoms), sum(num_atoms)
    lengths = lo + (hi - lo) * torch.rand(B, 3, generator=g)
    angles = ang[0] + (ang[1] - ang[0]) * torch.rand(B, 3, generator=g)
    lat = O.lattice_params_to_matrix(lengths, angles)
    frac = torch.rand(N, 3, generator=g)
    return frac, lat


@pytest.mark.parametrize("seed,num_atoms", [(1, [1, 2, 3, 20, 7]), (2, [20] * 6), (3, [5, 1, 1, 12, 30, 2, 9]), (4, [64, 3]),
                                            (5, [16, 16, 16, 8])])
def test_knn_graph_vs_oracle(seed, num_atoms):
    """Ragged batches incl. single-atom crystals (self-image edges only), dense cells where the max-neighbour trim
    is active, and the 64-atom limit."""
    frac, lat = _random_crystals(seed, num_atoms)
    na = torch.tensor(num_atoms)
    edges_ref, vec_ref = O.knn_edges(frac, lat, na, 20)
    net = _net(64, 1, 4)
    b = net.make_batch(num_atoms)
    E = b.build_graph(frac, lat)
    assert E == edges_ref.shape[1]
    edges, vec = b.edges("reference")
    assert edges.cpu().tolist() == edges_ref.tolist()
    np.testing.assert_array_equal(vec.cpu().numpy(), vec_ref.numpy())
    _check_csr(b, edges_ref, vec_ref, sum(num_atoms))


def test_knn_graph_symmetric_cells():
    """High-symmetry input: cubic cells with atoms on a 1/4 grid -> many exactly degenerate distances, shells that straddle
    the max-neighbour rank (the +0.01 band keeps whole shells), self-image edges at exactly the lattice constant."""
    num_atoms = [8, 4, 2, 1]
    lat = torch.stack([torch.eye(3) * a for a in (4.0, 5.5, 3.0, 2.5)])
    g = torch.Generator().manual_seed(11)
    frac = torch.randint(0, 4, (sum(num_atoms), 3), generator=g).float() / 4
    # distinct sites inside each crystal
    frac = torch.cat([torch.tensor([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.25, .25, .25], [.75, .75, .25], [.75, .25, .75],
                                    [.25, .75, .75]]), torch.tensor([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]]),
                      torch.tensor([[0, 0, 0], [.5, .5, .5]]), torch.tensor([[.1, .2, .3]])]).float()
    na = torch.tensor(num_atoms)
    edges_ref, vec_ref = O.knn_edges(frac, lat, na, 20)
    net = _net(64, 1, 4)
    b = net.make_batch(num_atoms)
    b.build_graph(frac, lat)
    edges, vec = b.edges("reference")
    assert edges.cpu().tolist() == edges_ref.tolist()
    np.testing.assert_array_equal(vec.cpu().numpy(), vec_ref.numpy())


def test_knn_capacity_error():
    """Exceeding the per-atom capacity raises; it never truncates silently."""
    from matinvent_amd.cspnet import CrystalBatch
    net = _net(64, 1, 4)
    frac, lat = _random_crystals(2, [20] * 2)
    b = CrystalBatch(net, [20, 20], edge_style="knn", max_neighbors=20, edge_cap_per_node=4)
    with pytest.raises(RuntimeError, match="capacity"):
        b.build_graph(frac, lat)


def test_knn_forward_and_grads_vs_oracle():
    """Forward outputs and dLoss/dtheta through the knn graph (general CSR edge list: gathers, segmented mean,
    in-edge sums of the backward) against the oracle's autograd."""
    H, L, F = 64, 2, 8
    num_atoms = [6, 20, 1, 11]
    frac, lat = _random_crystals(21, num_atoms)
    na = torch.tensor(num_atoms)
    B, N = len(num_atoms), sum(num_atoms)
    g = torch.Generator().manual_seed(5)
    at = torch.randn(N, 100, generator=g)
    t_emb = torch.randn(B, 256, generator=g)
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F, edge_style="knn")
    P = O.init_params(hp, seed=3)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    n2g = torch.repeat_interleave(torch.arange(B), na)
    pl, px, pt = O.cspnet_forward(Pg, hp, t_emb, at, frac, lat, na, n2g)
    wl, wx, wt = torch.randn(pl.shape, generator=g), torch.randn(px.shape, generator=g), torch.randn(pt.shape, generator=g)
    loss = (pl * wl).sum() + (px * wx).sum() + (pt * wt).sum()
    loss.backward()

    net = _net(H, L, F, P)
    net.theta.requires_grad_(True)
    b = net.make_batch(num_atoms)
    with torch.enable_grad():
        ql, qx, qt = net(t_emb.cuda(), at.cuda(), frac.cuda(), lat.cuda(), None, batch=b)
        (ql * wl.cuda()).sum().add((qx * wx.cuda()).sum()).add((qt * wt.cuda()).sum()).backward()
    _close(ql, pl, 2e-5, "pred_l")
    _close(qx, px, 2e-5, "pred_x")
    _close(qt, pt, 2e-5, "pred_t")
    gv = {k: net.theta.grad[o:o + n].view(shape).cpu() for k, (o, n, shape) in net.layout.items()}
    for k, v in gv.items():
        ref = Pg["decoder." + k].grad
        scale = max(float(ref.abs().max()), 1e-3)
        err = float((v - ref).abs().max())
        assert err <= 5e-4 * scale, f"grad {k}: {err:.3e} vs scale {scale:.3e}"


def test_knn_sample_chain_vs_oracle():
    """Free-running reverse chain with the graph rebuilt before every network evaluation (counter-based noise shared
    with the oracle).  The chain starts from N(0,1) lattices, i.e. arbitrary skewed cells."""
    from matinvent_amd.diffcsp import DiffCSPModule
    from tests.gpu_util import Box, wrap_dist
    T, seed = 8, 77
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8, edge_style="knn")
    P = O.init_params(hp, seed=1, head_scale=0.1)
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(T, generator=torch.Generator().manual_seed(3))])
    m = DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="knn", max_neighbors=20),
                      beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                      sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=sn), device="cuda")
    load_decoder(m.decoder, P)
    sch = O.Schedules.make(T, sigmas_norm=sn)
    na = torch.tensor([4, 9, 2, 12])
    noise = O.philox_sampler_noise(seed, na, T)
    of, _ = O.sample(P, hp, sch, na, noise, step_lr=5e-6)
    final, _ = m.sample(Box(na), step_lr=5e-6, seed=seed)
    assert wrap_dist(final["frac_coords"].cpu().numpy(), of["frac_coords"].numpy()).max() < 3e-4
    np.testing.assert_allclose(final["lattices"].cpu().numpy(), of["lattices"].numpy(), rtol=3e-4, atol=3e-4)
    np.testing.assert_allclose(final["atom_types"].cpu().numpy(), of["atom_types"].numpy(), rtol=3e-4, atol=3e-4)


def test_structure_check_vs_oracle():
    """K18: longest cell edge / shortest interatomic distance over 27 images / volume per crystal, against the oracle,
    incl. single-atom crystals (only self images) and the mask thresholds of the validity pre-filter."""
    from matinvent_amd.structure import check_structures, geometric_mask
    num_atoms = [1, 2, 20, 7, 33]
    frac, lat = _random_crystals(8, num_atoms, lo=2.0, hi=30.0)
    frac[1] = frac[2] + torch.tensor([0.01, 0.0, 0.0])  # crystal 1: an overlapping pair
    net = _net(64, 1, 4)
    b = net.make_batch(num_atoms)
    out = check_structures(b, frac.cuda(), lat.cuda()).cpu()
    ref = O.structure_check(frac, lat, torch.tensor(num_atoms))
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=2e-5, atol=1e-6)
    assert geometric_mask(out).tolist() == geometric_mask(ref).tolist()
    assert not bool(geometric_mask(out)[1])


def _knn_module(T, sn, P, **dec):
    from matinvent_amd.diffcsp import DiffCSPModule
    m = DiffCSPModule(decoder=dict(dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="knn", max_neighbors=20), **dec),
                      beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                      sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=sn), device="cuda")
    load_decoder(m.decoder, P)
    return m


def test_knn_chain_without_a_host_round_trip_equals_the_synchronising_chain_and_does_not_synchronise():
    """Inside mi_sampler_run every evaluation rebuilds the periodic neighbour list WITHOUT a host synchronisation (round 6): the consumers are launched for the
    list's capacity and read the edge count on the device.  (1) A recorded chain is bit for bit the chain of the synchronising build (mi_debug_set_knn_nosync(0));
    (2) a chain is enqueued while a long-running kernel still occupies the stream -- the reference synchronises twice per denoising step here
    (cspnet.py:243-257 -> utils.py:335-514: nonzero / masked_select)."""
    import time
    from matinvent_amd import _lib
    from tests.gpu_util import Box
    lib = _lib.load()
    T, seed = 8, 41
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8, edge_style="knn")
    P = O.init_params(hp, seed=1, head_scale=0.1)
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(T, generator=torch.Generator().manual_seed(3))])
    m = _knn_module(T, sn, P)
    na = torch.tensor([4, 9, 2, 12, 20, 1, 7])
    was = lib.mi_debug_set_knn_nosync(0)
    try:
        f0, t0 = m.sample(Box(na), step_lr=5e-6, seed=seed, record=True)
        trajs = []
        for mode in (1, 2):   # 1: the first build of the handle synchronises once (form hint), 2: none does
            lib.mi_debug_set_knn_nosync(mode)
            trajs.append(m.sample(Box(na), step_lr=5e-6, seed=seed, record=True)[1])
            m.check_graph()
    finally:
        lib.mi_debug_set_knn_nosync(was)
    for t1 in trajs:
        assert sorted(t0) == sorted(t1)
        for t in t0:
            for k in t0[t]:
                assert torch.equal(t0[t][k], t1[t][k]), (t, k)
    # (2) no synchronisation inside the enqueue
    box = Box(na)
    m.sample(box, step_lr=5e-6, seed=1)
    m.check_graph()
    torch.cuda.synchronize()
    _lib.check(lib.mi_debug_spin(int(2.0e9), None))  # ~1 s of busy-wait on the null stream ahead of the chain
    t_start = time.perf_counter()
    m.sample(box, step_lr=5e-6, seed=2)
    t_enqueue = time.perf_counter() - t_start
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t_start
    m.check_graph()
    assert t_total > 0.3 and t_enqueue < 0.5 * t_total, (t_enqueue, t_total)


def test_knn_capacity_error_inside_a_chain_is_raised_behind_it():
    """A list over capacity cannot raise in the middle of an enqueued chain: it contributes no edges, sets a sticky flag, and check_graph() -- which sample() runs
    for the previous call's chains and DiffCSPSampler.generate before it unpacks -- raises the same capacity error.  Never a silent truncation."""
    from matinvent_amd import _lib
    from tests.gpu_util import Box
    lib = _lib.load()
    T = 4
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8, edge_style="knn")
    P = O.init_params(hp, seed=1, head_scale=0.1)
    m = _knn_module(T, torch.ones(T + 1), P)
    m.decoder.edge_cap_per_node = 4
    box = Box(torch.tensor([20, 20]))
    # the very first build of a batch handle synchronises once (the host learns the list's size): an overflow there raises at once
    with pytest.raises(RuntimeError, match="capacity"):
        m.sample(box, step_lr=5e-6, seed=3)
    was = lib.mi_debug_set_knn_nosync(2)          # no synchronisation at all: what every LATER build of a handle does
    try:
        m.sample(box, step_lr=5e-6, seed=3)      # enqueues; dense 20-atom cells overflow 4 kept neighbours per atom at once
        with pytest.raises(RuntimeError, match="capacity"):
            m.check_graph()
        m.check_graph()                           # (the flag was cleared with the report)
        m.sample(box, step_lr=5e-6, seed=4)
        with pytest.raises(RuntimeError, match="capacity"):
            m.sample(box, step_lr=5e-6, seed=5)  # the next call reports the previous call's chains first
        # with the error reported, the handle describes no list (it used to go on reporting the capacity, 2 x 4 x 40 rows of stale edges)
        cb = m.crystal_batch(box)
        assert int(lib.mi_batch_num_edges(cb._h)) == 0 and cb.num_edges == 0
        assert cb.edges("reference")[0].shape == (2, 0) and cb.edges("csr")[1].shape == (0, 3)
        # ... and is as good as new: one step from a geometry INSIDE the capacity (skewed N(0,1) cells, coordinates in the home cell as the chain
        # keeps them: at most 2 edges per atom, checked with the oracle right here) is bit for bit the step on a fresh handle -- the over-capacity
        # builds left no row span, degree or table behind
        from tests import knn_cases as K
        frac, lat = K.sparse([20, 20], 251)
        frac = frac % 1.0
        edges_ref, _ = O.knn_edges(frac, lat, box.num_atoms, 20)
        assert 0 < K.max_degree(edges_ref, 40) <= 2 < m.decoder.edge_cap_per_node and K.margin(frac, lat, [20, 20]) > 1e-2
        init = (frac, lat, torch.randn(40, 100, generator=torch.Generator().manual_seed(9)))
        runs = []
        for bx in (box, Box(torch.tensor([20, 20]))):
            _, traj = m.sample(bx, step_lr=5e-6, seed=6, init=init, t_start=1, t_stop=0, record=True)
            m.check_graph()                       # (inside the capacity on the device as well)
            runs.append(traj)
        assert m.crystal_batch(box) is cb and int(lib.mi_batch_num_edges(cb._h)) > 0
        for t in runs[0]:
            for k in ("atom_types", "frac_coords", "lattices"):
                assert torch.equal(runs[0][t][k], runs[1][t][k]), (t, k)
    finally:
        lib.mi_debug_set_knn_nosync(was)
        m.__dict__["_knn_pending"] = []
