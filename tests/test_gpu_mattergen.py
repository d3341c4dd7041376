"""GPU checks of the MatterGen-shaped path (csrc/gemnet.hip through the C ABI and the host mirror matinvent_amd/mattergen.py)
against oracle/mattergen_oracle.py.  SELF-CONSISTENT, PARITY-UNPINNED vs upstream: the reference's MatterGen arithmetic lives in
the un-vendored package mattergen @ 5bb2b397; the oracle restates the published algorithms and is what these tests compare with."""
import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as DO
from oracle import mattergen_oracle as M

pytestmark = pytest.mark.gpu


def _module(hp_dict, P=None, **kw):
    from matinvent_amd.mattergen import MatterGenModule
    g = {k: v for k, v in hp_dict.items()}
    m = MatterGenModule(gemnet=g, **kw)
    if P is not None:
        m.decoder.load_state_dict(P, strict=True)
    return m


def _case(na, seed=1, cell_scale=5.0, jitter=0.5):
    g = torch.Generator().manual_seed(seed)
    na = torch.tensor(na)
    N, B = int(na.sum()), len(na)
    frac = torch.rand(N, 3, generator=g)
    cell = cell_scale * torch.eye(3)[None].repeat(B, 1, 1) + jitter * M.symmetric_noise(torch.randn(B, 3, 3, generator=g))
    a = torch.randint(1, 101, (N,), generator=g)
    a[::5] = M.MASK
    t = 0.1 + 0.8 * torch.rand(B, generator=g)
    return na, frac, cell, a, t, g


def _rel(a, b, tol, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    scale = max(1e-12, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.0e} * max|ref| ({scale:.3g})"


def test_parameter_layout_matches_the_oracle_list():
    hp = M.GemNetHParams(**M.TINY)
    m = _module(M.TINY)
    names = [(n, r, c) for n, r, c in M.param_list(hp)]
    assert [n for n, _, _ in names] == list(m.decoder.layout.keys())
    for (n, r, c), (k, (off, numel, shape)) in zip(names, m.decoder.layout.items()):
        assert numel == r * c and off % 4 == 0, n
    big = M.GemNetHParams()
    assert sum(r * c for _, r, c in M.param_list(big)) == 42722427   # the 512-wide network of THIS restatement (upstream: ~46.8 M [UPSTREAM-UNVERIFIED]; 28.3 M before the
    # output blocks took upstream's shape: energy path, num_atom residual layers on the force path, ScalingFactors -- round 5)


@pytest.mark.parametrize("na,scale,hpk", [([4, 7, 1, 10], 5.0, {}), ([20, 20, 3], 3.2, dict(max_neighbors=12)), ([2, 5], 2.0, dict(cutoff=6.0, max_images=4))])
def test_periodic_graph_matches_the_oracle_exactly(na, scale, hpk):
    """Integer work: the edge list (sources, targets, images, reverse-edge index, row pointers) must be IDENTICAL, including small
    cells that need several periodic images per dimension and single-atom crystals that only see their own images."""
    hpd = dict(M.TINY, **hpk)
    hp = M.GemNetHParams(**hpd)
    m = _module(hpd)
    na, frac, cell, a, t, g = _case(na, seed=3, cell_scale=scale)
    og = M.build_graph(frac, cell, na, hp)
    gb = m.decoder.make_batch(na)
    dg = gb.graph(frac, cell)
    for k in ("src", "dst", "img", "swap", "rowptr"):
        assert torch.equal(dg[k].cpu(), og[k]), k
    _rel(dg["D"], og["D"], 1e-6, "D")
    _rel(dg["V"], og["V"], 2e-6, "V")
    E = len(og["src"])
    assert E > 0 and torch.equal(og["swap"][og["swap"]], torch.arange(E))


# the benchmark network's basis sizes (7 spherical orders, 16-wide circular basis, 64-wide triplet embedding: the branches of the triplet
# kernels that the four-order TINY network does not reach) at widths the CPU oracle finishes in seconds
BASIS7 = dict(M.TINY, emb_trip=64, emb_cbf=16, emb_rbf=16, emb_bil=64, num_spherical=7, num_radial=32)
# GemNet's ScalingFactors with FITTED values (upstream ships them as constants of the checkpoint; identity-initialised here) and two residual layers
# in the output blocks' stacks: the elementwise pass of op_scale and its gradient, which the identity case never launches
FITTED = dict(M.TINY, num_atom=2)
CASES = [(M.TINY, False), (BASIS7, False), (FITTED, True)]
CASE_IDS = ["tiny", "benchmark-basis-sizes", "fitted-scale-factors"]


def _fit_scale_factors(P, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in P:
        if M.is_scale_factor(k):
            P[k] = 0.6 + 0.9 * torch.rand(1, 1, generator=g)
    return P


@pytest.mark.parametrize("hpd,fitted", CASES, ids=CASE_IDS)
def test_forward_matches_the_oracle_layer_by_layer(hpd, fitted):
    hp = M.GemNetHParams(**hpd)
    P = M.init_params(hp, seed=0, head_scale=0.3)
    if fitted:
        P = _fit_scale_factors(P)
    m = _module(hpd, P)
    na, frac, cell, a, t, g = _case([4, 7, 1, 10, 20])
    taps = {}
    ref = M.gemnet_forward(P, hp, frac, cell, a, na, t, taps=taps)
    gb = m.decoder.make_batch(na)
    with torch.no_grad():
        out = m.decoder(frac, cell, a, t, gb)
    _rel(gb.tap("rbf"), taps["rbf"].reshape(-1), 5e-6, "rbf")   # (device expf vs libm on Gaussians up to exp(-60): 2.3e-6 measured at 32 radial functions)
    _rel(gb.tap("h0"), taps["h0"].reshape(-1), 1e-5, "h0")
    _rel(gb.tap("m0"), taps["m0"].reshape(-1), 1e-5, "m0")
    for i in range(hp.num_blocks):
        _rel(gb.tap(f"x3_{i}"), taps[f"x3_{i}"].reshape(-1), 2e-5, f"x3_{i}")
        _rel(gb.tap(f"h{i + 1}"), taps[f"h{i + 1}"].reshape(-1), 2e-5, f"h{i + 1}")
        _rel(gb.tap(f"m{i + 1}"), taps[f"m{i + 1}"].reshape(-1), 2e-5, f"m{i + 1}")
    for k in ("pos", "cell", "atomic_numbers"):
        _rel(out[k], ref[k], 2e-5, k)
    # bit-reproducible: a second evaluation gives the same bits (fixed reduction orders, no float atomics)
    with torch.no_grad():
        out2 = m.decoder(frac, cell, a, t, gb)
    for k in out:
        assert torch.equal(out[k], out2[k]), k


@pytest.mark.parametrize("hpd,fitted", CASES, ids=CASE_IDS)
def test_parameter_gradients_match_the_oracle_autograd(hpd, fitted):
    hp = M.GemNetHParams(**hpd)
    P = M.init_params(hp, seed=2, head_scale=0.5)
    if fitted:
        P = _fit_scale_factors(P)
    m = _module(hpd, P)
    na, frac, cell, a, t, g = _case([5, 1, 12, 20, 3], seed=7)
    N, B = int(na.sum()), len(na)
    up, uc, ul = torch.randn(N, 3, generator=g), M.symmetric_noise(torch.randn(B, 3, 3, generator=g)), torch.randn(N, 101, generator=g)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = M.gemnet_forward(Pg, hp, frac, cell, a, na, t)
    ((ref["pos"] * up).sum() + (ref["cell"] * uc).sum() + (ref["atomic_numbers"] * ul).sum()).backward()
    gb = m.decoder.make_batch(na)
    out = m.decoder(frac, cell, a, t, gb)
    ((out["pos"] * up.cuda()).sum() + (out["cell"] * uc.cuda()).sum() + (out["atomic_numbers"] * ul.cuda()).sum()).backward()
    th = m.decoder.theta
    unused = 0
    for k, (o, n, shape) in m.decoder.layout.items():
        if Pg[k].grad is None:   # the energy path (E_t feeds no output) and the ScalingFactors (constants): no gradient on either side
            assert M.is_scale_factor(k) or ".seq_energy." in k or ".out_energy." in k or ".dense_rbf." in k or ".scale_sum." in k, k
            assert not bool(th.grad[o:o + n].any()), k
            unused += 1
            continue
        _rel(th.grad[o:o + n].view(shape), Pg[k].grad, 5e-5, f"grad {k}")
    assert unused > 0
    # `+=` semantics across backward calls, like .grad
    g1 = th.grad.clone()
    out = m.decoder(frac, cell, a, t, gb)
    ((out["pos"] * up.cuda()).sum() + (out["cell"] * uc.cuda()).sum() + (out["atomic_numbers"] * ul.cuda()).sum()).backward()
    assert torch.allclose(th.grad, 2 * g1, rtol=1e-5, atol=1e-7)


def _batch_obj(na, frac, cell, a):
    from matinvent_amd.mattergen import ChemGraph, ChemGraphBatch
    off = [0] + torch.cumsum(na, 0).tolist()
    return ChemGraphBatch([ChemGraph(frac[off[i]:off[i + 1]], cell[i:i + 1], a[off[i]:off[i + 1]]) for i in range(len(na))])


def test_add_noise_loss_and_anchor_penalty_match_the_oracle():
    """The adapter surface (pl_module.py:55-102, loss.py:36-78): time grid, sample_marginal, per-sample weighted loss, anchor penalty."""
    hp = M.GemNetHParams(**M.TINY)
    P, Q = M.init_params(hp, seed=0, head_scale=0.3), M.init_params(hp, seed=1, head_scale=0.3)
    agent, prior = _module(M.TINY, P), _module(M.TINY, Q)
    na, frac, cell, a, _, g = _case([4, 7, 1, 10], seed=11)
    a = torch.randint(1, 101, a.shape, generator=g)
    N, B = int(na.sum()), len(na)
    batch = _batch_obj(na, frac, cell, a)
    corr = M.Corruption()
    ob = dict(pos=frac, cell=cell, atomic_numbers=a, num_atoms=na)
    for ti in (0, 400, 999):
        nz = (torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g), torch.rand(N, generator=g))
        t = torch.full((B,), M.time_grid(corr, ti))
        noisy_o, aux = M.sample_marginal(corr, ob, t, dict(pos=nz[0], cell=nz[1], types=nz[2]))
        pred_o = M.gemnet_forward(P, hp, noisy_o["pos"], noisy_o["cell"], noisy_o["atomic_numbers"], na, t)
        loss_o, _ = M.sample_loss(corr, ob, aux, pred_o)
        pq = M.gemnet_forward(Q, hp, noisy_o["pos"], noisy_o["cell"], noisy_o["atomic_numbers"], na, t)
        kl_o = M.calc_kl_reg(pred_o, pq, aux["node2graph"], B)
        with torch.no_grad():
            noised = agent.add_noise(batch, ti, noise=nz)
            noisy, _, tt = noised
            d = np.abs(noisy["pos"].cpu().numpy() - noisy_o["pos"].numpy())
            assert np.minimum(d, 1 - d).max() < 2e-6, ti
            _rel(noisy["cell"], noisy_o["cell"], 2e-6, "noisy cell")
            assert torch.equal(noisy["atomic_numbers"].cpu(), noisy_o["atomic_numbers"])
            _rel(tt, t, 1e-7, "t")
            loss, pred = agent.calc_sample_loss(noised)
            _, ppred = prior.calc_sample_loss(noised)
            kl = agent.calc_kl_reg(pred, ppred, batch)
        _rel(loss, loss_o, 5e-5, f"sample loss t{ti}")
        _rel(kl, kl_o, 2e-4, f"kl t{ti}")


def _pc_noise(N, B, n, g):
    return dict(init_pos=torch.rand(N, 3, generator=g), init_cell=torch.randn(B, 3, 3, generator=g),
                corr_pos=[torch.randn(N, 3, generator=g) for _ in range(n)], corr_cell=[torch.randn(B, 3, 3, generator=g) for _ in range(n)],
                pred_pos=[torch.randn(N, 3, generator=g) for _ in range(n)], pred_cell=[torch.randn(B, 3, 3, generator=g) for _ in range(n)],
                pred_u1=[torch.rand(N, generator=g) for _ in range(n)], pred_u2=[torch.rand(N, generator=g) for _ in range(n)])


def test_predictor_corrector_steps_match_the_oracle():
    """Teacher-forced steps of the 1000-point grid with injected noise, resumed from a given state at late grid points (small t: at
    t ~ 1 the positions are re-drawn over several cell lengths per step and the neighbour selection flips under 1e-6 perturbations, so a
    step there is not a continuous function of its input -- measured on the oracle itself), and the D3PM reveal rule on a short grid.
    The returned MEAN batch (what MatterGenSampler hands on, sample.py:49-50) and the state are compared."""
    hp = M.GemNetHParams(**M.TINY)
    P = M.init_params(hp, seed=4, head_scale=20.0)   # outputs of order one, like a trained denoiser's score x std
    m = _module(M.TINY, P)
    # (no single-atom crystal here: its position score is an exact zero in real arithmetic -- every edge has its mirror image -- so
    # the signal-to-noise step size divides by round-off)
    na = torch.tensor([4, 6, 3, 9])
    N, B = int(na.sum()), len(na)
    corr = M.Corruption()
    g = torch.Generator().manual_seed(5)
    for start in (995, 990, 970, 950, 900):
        state = dict(pos=torch.rand(N, 3, generator=g), cell=4.5 * torch.eye(3)[None].repeat(B, 1, 1) + 0.3 * M.symmetric_noise(torch.randn(B, 3, 3, generator=g)),
                     atomic_numbers=torch.randint(1, 102, (N,), generator=g))
        stop = start + 1   # single steps: chained steps multiply the step's own (large, random-network) Lipschitz constant
        raw = _pc_noise(N, B, 1, g)
        nz_o = {k: ([None] * start + v if isinstance(v, list) else v) for k, v in raw.items()}   # the oracle indexes noise by grid point
        nz_d = {k: ([torch.zeros_like(v[0])] * start + v if isinstance(v, list) else v) for k, v in raw.items()}
        so, mo = M.pc_sample(P, hp, corr, na, nz_o, n_steps=1000, t_stop_index=stop, start_index=start, state=state)
        s, mean = m.sample(na, n_steps=1000, noise=nz_d, i_stop=stop, i_start=start, state=state)
        d = np.abs(mean["pos"].cpu().numpy() - mo["pos"].numpy())
        assert np.minimum(d, 1 - d).max() < 1e-4, (start, np.minimum(d, 1 - d).max())
        d = np.abs(s["pos"].cpu().numpy() - so["pos"].numpy())
        assert np.minimum(d, 1 - d).max() < 1e-4, (start, np.minimum(d, 1 - d).max())
        _rel(mean["cell"], mo["cell"], 1e-4, f"mean cell {start}")
        _rel(s["cell"], so["cell"], 1e-4, f"cell {start}")
        assert torch.equal(s["atomic_numbers"].cpu(), so["atomic_numbers"]), start
    # D3PM reveal on the last grid points: tau = 1 at the end reveals every remaining mask
    state = dict(pos=torch.rand(N, 3, generator=g), cell=4.5 * torch.eye(3)[None].repeat(B, 1, 1), atomic_numbers=torch.full((N,), M.MASK))
    raw = _pc_noise(N, B, 4, g)
    nz_o = {k: ([None] * 996 + v if isinstance(v, list) else v) for k, v in raw.items()}
    nz_d = {k: ([torch.zeros_like(v[0])] * 996 + v if isinstance(v, list) else v) for k, v in raw.items()}
    so, mo = M.pc_sample(P, hp, corr, na, nz_o, n_steps=1000, start_index=996, state=state)
    s, mean = m.sample(na, n_steps=1000, noise=nz_d, i_start=996, state=state)
    assert torch.equal(s["atomic_numbers"].cpu(), so["atomic_numbers"]) and int((s["atomic_numbers"] == M.MASK).sum()) == 0


def test_philox_chain_is_shard_invariant_and_reproducible():
    """Built-in counter-based noise: the same chain twice gives the same bits; sampling the crystals in two shards with global
    offsets gives the samples of the unsplit batch."""
    hp = M.GemNetHParams(**M.TINY)
    m = _module(M.TINY, M.init_params(hp, seed=6, head_scale=20.0))
    na = [4, 6, 1, 9, 5]
    s1, m1 = m.sample(na, n_steps=1000, seed=9, i_stop=2)
    s2, m2 = m.sample(na, n_steps=1000, seed=9, i_stop=2)
    assert bool(torch.isfinite(m1["pos"]).all()) and bool(torch.isfinite(m1["cell"]).all())
    for k in ("pos", "cell"):
        assert torch.equal(m1[k], m2[k])
    sa, ma = m.sample(na[:2], n_steps=1000, seed=9, i_stop=2)
    sb, mb = m.sample(na[2:], n_steps=1000, seed=9, i_stop=2, node_offset=10, graph_offset=2)
    assert torch.allclose(torch.cat([ma["cell"], mb["cell"]]), m1["cell"], rtol=1e-5, atol=1e-6)
    d = (torch.cat([ma["pos"], mb["pos"]]) - m1["pos"]).abs()
    assert float(torch.minimum(d, 1 - d).max()) < 1e-5


def test_concurrent_chains_reproduce_the_single_chain():
    """`chains` > 1 samples contiguous crystal groups concurrently on separate streams (each with its own batch handle; whichever chain
    meets a weight block first builds its plane set under the network's mutex, the others wait for the block's event), at a size where
    the plane-set layers run.  Bit for bit the samples of the same groups
    sampled one after the other (no race between the chains); against the UNSPLIT batch they agree to what the plane format's rounding
    leaves after three steps of a random-init chain -- the power-of-two scales of the plane sets come from batch-wide maxima, so the
    22-bit rounding of an edge-level tensor depends on which crystals share a batch (measured 4e-4 of max|cell|)."""
    hpd = dict(M.TINY, emb_atom=128, emb_edge=128)
    hp = M.GemNetHParams(**hpd)
    m = _module(hpd, M.init_params(hp, seed=6, head_scale=20.0))
    na = [20] * 40 + [7, 12, 1, 20]
    s1, m1 = m.sample(na, n_steps=1000, seed=9, i_stop=3)
    for chains in (2, 3):
        m.decoder._dirty = True   # (a parameter upload: the library rebuilds its weight plane sets)
        s2, m2 = m.sample(na, n_steps=1000, seed=9, i_stop=3, chains=chains)
        cuts = [len(na) * k // chains for k in range(chains + 1)]
        seq = [m.sample(na[cuts[k]:cuts[k + 1]], n_steps=1000, seed=9, i_stop=3, node_offset=sum(na[:cuts[k]]), graph_offset=cuts[k])[1] for k in range(chains)]
        for key in ("pos", "cell", "atomic_numbers", "num_atoms"):
            assert torch.equal(torch.cat([p[key] for p in seq]), m2[key]), (chains, key)
        assert torch.equal(s1["atomic_numbers"], s2["atomic_numbers"])
        assert float((m2["cell"] - m1["cell"]).abs().max()) <= 2e-3 * float(m1["cell"].abs().max()), chains
        # (positions are not compared with the unsplit batch: at t ~ 1 a step re-draws them over several cell lengths and is not a
        #  continuous function of its input -- DESIGN section 11 -- so a rounding difference moves single atoms by O(1))


def test_sampler_without_a_host_round_trip_equals_the_synchronising_form():
    """The chain's forwards keep the graph's edge count on the device (mi_gemnet_forward bit 2: launches sized by the capacity, the
    count read from meta[0], a compact activation arena sized once per handle).  Same kernels on the same rows in the same order as the
    form that synchronises once per evaluation to read the count: the samples must agree BIT FOR BIT, at a size where the plane-set
    layers run in both forms (6.7 k edges, capacity 13.4 k)."""
    from matinvent_amd import _lib
    lib = _lib.load()
    hpd = dict(M.TINY, emb_atom=128, emb_edge=128)
    hp = M.GemNetHParams(**hpd)
    m = _module(hpd, M.init_params(hp, seed=6, head_scale=20.0))
    na = [20] * 40 + [7, 12, 1, 20]
    try:
        lib.mi_debug_set_mg_nosync(0)
        s0, m0 = m.sample(na, n_steps=1000, seed=9, i_stop=3)
        lib.mi_debug_set_mg_nosync(1)
        s1, m1 = m.sample(na, n_steps=1000, seed=9, i_stop=3)
        inv = m.last_sample_invalid()
        s2, m2 = m.sample(na, n_steps=1000, seed=9, i_stop=3)   # (second call: the program's dry passes come from the handle's cache)
    finally:
        lib.mi_debug_set_mg_nosync(1)
    assert inv.shape == (len(na),) and not bool(inv.any())
    for key in ("pos", "cell", "atomic_numbers"):
        assert torch.equal(m0[key], m1[key]) and torch.equal(s0[key], s1[key]), key
        assert torch.equal(m1[key], m2[key]) and torch.equal(s1[key], s2[key]), key
    assert bool(torch.isfinite(m1["pos"]).all()) and bool(torch.isfinite(m1["cell"]).all())
    assert _lib.saturation_events(reset=True) == 0


def test_graph_read_after_a_sampler_run_without_a_host_round_trip_equals_the_synchronising_form():
    """The chain's forwards leave the CAPACITY as the handle's edge count (the real count stays on the device).  Once graph_status() has
    been asked -- last_sample_invalid() does -- the handle describes the last evaluation's graph: reading it returns the rows, and only
    the rows, that the synchronising form leaves (it used to copy capacity-many rows, most of them stale)."""
    from matinvent_amd import _lib
    lib = _lib.load()
    hpd = dict(M.TINY, emb_atom=128, emb_edge=128)
    hp = M.GemNetHParams(**hpd)
    m = _module(hpd, M.init_params(hp, seed=6, head_scale=20.0))
    na = [20] * 40 + [7, 12, 1, 20]
    graphs = []
    try:
        for mode in (0, 1):
            lib.mi_debug_set_mg_nosync(mode)
            m.sample(na, n_steps=1000, seed=9, i_stop=3)
            (gb,) = m._last_chain_batches
            if mode == 1:   # (the count is still on the device: no read of capacity-many rows)
                with pytest.raises(RuntimeError, match="mi_gbatch_graph_status"):
                    gb.read_graph()
            assert not bool(m.last_sample_invalid().any())
            graphs.append({k: v.clone() for k, v in gb.read_graph().items()})
    finally:
        lib.mi_debug_set_mg_nosync(1)
    g0, g1 = graphs
    E = g0["src"].shape[0]
    assert 0 < E == int(g0["rowptr"][-1]) < sum(na) * 2 * hp.max_neighbors
    for k in ("src", "dst", "img", "swap", "rowptr", "D", "V"):
        assert g1[k].shape == g0[k].shape and torch.equal(g1[k], g0[k]), k


def test_sampler_with_fitted_scale_factors_takes_the_synchronising_form():
    """GemNet's ScalingFactors with values other than one are elementwise passes on fp32 rows (op_scale), which the plane-only program of the
    no-round-trip forwards does not have: the chain then runs on the synchronising form whatever mi_debug_set_mg_nosync says (same samples both ways,
    finite, reproducible), and differs from the identity-factor chain."""
    from matinvent_amd import _lib
    lib = _lib.load()
    hpd = dict(M.TINY, emb_atom=128, emb_edge=128)
    hp = M.GemNetHParams(**hpd)
    P = M.init_params(hp, seed=6, head_scale=20.0)
    m1 = _module(hpd, P)
    na = [20] * 40 + [7, 12, 1, 20]
    s_id, m_id = m1.sample(na, n_steps=1000, seed=9, i_stop=2)
    mf = _module(hpd, _fit_scale_factors({k: v.clone() for k, v in P.items()}))
    try:
        lib.mi_debug_set_mg_nosync(1)
        sa, ma = mf.sample(na, n_steps=1000, seed=9, i_stop=2)
        assert not bool(mf.last_sample_invalid().any())
        lib.mi_debug_set_mg_nosync(0)
        sb, mb = mf.sample(na, n_steps=1000, seed=9, i_stop=2)
    finally:
        lib.mi_debug_set_mg_nosync(1)
    for key in ("pos", "cell", "atomic_numbers"):
        assert torch.equal(ma[key], mb[key]) and torch.equal(sa[key], sb[key]), key
    assert bool(torch.isfinite(ma["pos"]).all()) and bool(torch.isfinite(ma["cell"]).all())
    assert not torch.equal(ma["cell"], m_id["cell"])


def test_a_crystal_over_a_graph_capacity_is_dropped_alone():
    """A crystal with an in-degree above the graph's capacity (128 in-edges, the triplet kernels' LDS image; lowered to 24 here so that a
    dense cell exceeds it -- a collapsed cell is what would do it in a chain) fails the synchronising forward as a whole (MI_ECAPACITY).
    The chain's forwards take that ONE crystal out of the graph on the device, remember its flag, and go on: the other crystals'
    samples are those of a batch that never held it, up to the plane format's batch-composition rounding (the reference drops
    collapsed crystals one by one after sampling, pipeline/filters/opt_filter.py:49-61)."""
    from matinvent_amd import _lib
    lib = _lib.load()
    hpd = dict(M.TINY, emb_atom=128, emb_edge=128, max_neighbors=32)
    hp = M.GemNetHParams(**hpd)
    m = _module(hpd, M.init_params(hp, seed=6, head_scale=20.0))
    g = torch.Generator().manual_seed(4)
    na = [20, 40, 40]
    N = sum(na)
    cell = torch.stack([2.4 * torch.eye(3), 13.0 * torch.eye(3), 13.5 * torch.eye(3)]) + 0.1 * M.symmetric_noise(torch.randn(3, 3, 3, generator=g))
    state = dict(pos=torch.rand(N, 3, generator=g).cuda(), cell=cell.cuda(), atomic_numbers=torch.randint(1, 101, (N,), generator=g).cuda())
    t = torch.full((3,), 0.1)
    kw = dict(n_steps=1000, seed=5, i_start=900, i_stop=901)
    try:
        lib.mi_debug_set_mg_deg_cap(24)
        with pytest.raises(_lib.MIError) as ei, torch.no_grad():
            m.decoder(state["pos"], state["cell"], state["atomic_numbers"], t, m.decoder.make_batch(torch.tensor(na)))
        assert ei.value.code == _lib.MI_ECAPACITY and "periodic graph" in str(ei.value)
        s_all, m_all = m.sample(na, state={k: v.clone() for k, v in state.items()}, **kw)
        inv = m.last_sample_invalid()
        assert inv.tolist() == [True, False, False]
        assert all(bool(torch.isfinite(m_all[k].float()).all()) for k in ("pos", "cell"))
        rest = dict(pos=state["pos"][20:].clone(), cell=state["cell"][1:].clone(), atomic_numbers=state["atomic_numbers"][20:].clone())
        s_r, m_r = m.sample(na[1:], state=rest, node_offset=20, graph_offset=1, **kw)
        assert not bool(m.last_sample_invalid().any())
    finally:
        lib.mi_debug_set_mg_deg_cap(0)
    assert torch.equal(m_all["atomic_numbers"][20:], m_r["atomic_numbers"])
    assert float((m_all["cell"][1:] - m_r["cell"]).abs().max()) <= 2e-3 * float(m_r["cell"].abs().max())
    d = (m_all["pos"][20:] - m_r["pos"]).abs()
    assert float(torch.minimum(d, 1 - d).median()) <= 1e-4


def test_fine_tune_step_through_the_pipeline_surface_vs_oracle():
    """matinvent_amd.finetune.ft_step on the MatterGen-shaped module (the reference's loop, pipeline/mat_invent.py:150-177, over
    add_noise / calc_sample_loss / calc_kl_reg, fused Adam on the flat parameter vector) against the same loop over the oracle with
    torch autograd: one accumulation window of 3 timesteps + the Adam step."""
    from matinvent_amd.finetune import ft_step
    from matinvent_amd.mattergen import ChemGraph, symmetrize_lattice
    hp = M.GemNetHParams(**M.TINY)
    P0, Q0 = M.init_params(hp, seed=0, head_scale=0.3), M.init_params(hp, seed=0, head_scale=0.3)
    g = torch.Generator().manual_seed(31)
    for k in P0:
        P0[k] = P0[k] + 0.01 * torch.randn(P0[k].shape, generator=g)
    agent, prior = _module(M.TINY, P0), _module(M.TINY, Q0)
    prior.requires_grad_(False)
    na, frac, cell, a, _, g = _case([4, 7, 2, 10], seed=13)
    a = torch.randint(1, 101, a.shape, generator=g)
    N, B = int(na.sum()), len(na)
    off = [0] + torch.cumsum(na, 0).tolist()
    data = [ChemGraph(frac[off[i]:off[i + 1]], cell[i:i + 1], a[off[i]:off[i + 1]]) for i in range(B)]
    rewards = torch.rand(B, generator=g).numpy()
    TS = 3
    noises = {(0, t): (torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g), torch.rand(N, generator=g)) for t in range(TS)}
    cfg = dict(lr=1e-4, accum_steps=TS, epochs=1, timesteps=TS, sigma=0.025)
    stats = ft_step(agent, prior, data, rewards, cfg, noise_fn=lambda e, t: noises[(e, t)])
    # oracle: the same loop (cells symmetrised by the dataset transform, like the product path)
    corr = M.Corruption()
    ob = dict(pos=frac, cell=symmetrize_lattice(cell), atomic_numbers=a, num_atoms=na)
    A = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    rw = torch.from_numpy(rewards).float()
    grads = {k: torch.zeros_like(v) for k, v in A.items()}
    tot = 0.0
    for ti in range(TS):
        t = torch.full((B,), M.time_grid(corr, ti))
        noisy, aux = M.sample_marginal(corr, ob, t, dict(zip(("pos", "cell", "types"), noises[(0, ti)])))
        pa = M.gemnet_forward(A, hp, noisy["pos"], noisy["cell"], noisy["atomic_numbers"], na, t)
        with torch.no_grad():
            pp = M.gemnet_forward(Q0, hp, noisy["pos"], noisy["cell"], noisy["atomic_numbers"], na, t)
        sl, _ = M.sample_loss(corr, ob, aux, pa)
        kl = M.calc_kl_reg(pa, pp, aux["node2graph"], B)
        loss = (rw * sl + 0.025 * kl * (1.1 - rw)).mean() / TS
        gs = M.param_grads(loss, A)
        for k, gg in zip(A, gs):
            grads[k] += gg
        tot += float(loss) * TS
    assert abs(stats[0]["loss"] - tot / TS) <= 1e-4 * max(1.0, abs(tot / TS)), (stats[0]["loss"], tot / TS)
    with torch.no_grad():
        Ad = {k: v.detach().clone() for k, v in A.items()}
        DO.adam_step(Ad, grads, {}, 1e-4)
    bad = tot_n = 0
    for k, w in agent.decoder.views().items():
        d = (w.detach().cpu() - Ad[k]).abs()
        assert float(d.max()) <= 2.1e-4, f"{k}: {float(d.max())}"
        bad += int((d > 1e-5).sum())
        tot_n += d.numel()
    assert bad <= 0.02 * tot_n, f"{bad} of {tot_n} parameters differ by more than 1e-5 after the Adam step"


def test_fine_tune_step_in_chunks_equals_the_unchunked_step(monkeypatch):
    """A fine-tune set larger than the activation budget is walked in chunks of crystals (equal-shaped chunks share one batch handle
    and its arenas; the noise is indexed by global ids and every chunk of a timestep draws from the same Philox step): the update
    must be the unchunked one up to the summation order of the gradient."""
    import matinvent_amd.mattergen as MG
    from matinvent_amd.finetune import ft_step
    from matinvent_amd.mattergen import ChemGraph
    hp = M.GemNetHParams(**M.TINY)
    g = torch.Generator().manual_seed(17)
    P0 = M.init_params(hp, seed=5, head_scale=0.3)
    na, frac, cell, a, _, g = _case([6, 6, 6, 6, 3, 9, 6], seed=19)
    a = torch.randint(1, 101, a.shape, generator=g)   # (clean records: elements only, no mask state)
    off = [0] + torch.cumsum(na, 0).tolist()
    data = [ChemGraph(frac[off[i]:off[i + 1]], cell[i:i + 1], a[off[i]:off[i + 1]]) for i in range(len(na))]
    rewards = torch.rand(len(na), generator=g).numpy()
    cfg = dict(lr=1e-4, accum_steps=2, epochs=1, timesteps=3, sigma=0.025)
    out = []
    for limit in (10 ** 9, 12):   # one chunk; chunks of two 6-atom crystals (one shared handle), then [3, 9], then [6]
        monkeypatch.setattr(MG, "FT_CHUNK_ATOMS", limit)
        agent, prior = _module(M.TINY, P0), _module(M.TINY, P0)
        prior.requires_grad_(False)
        agent.noise_seed = prior.noise_seed = 77
        stats = ft_step(agent, prior, data, rewards, cfg)
        out.append((stats[0], {k: v.detach().cpu().clone() for k, v in agent.decoder.views().items()}))
    (s0, w0), (s1, w1) = out
    assert abs(s0["loss"] - s1["loss"]) <= 1e-5 * max(1.0, abs(s0["loss"])), (s0, s1)
    for k in w0:
        assert float((w0[k] - w1[k]).abs().max()) <= 2e-6, k   # (lr 1e-4: an Adam step moves a weight by at most ~1e-4)


@pytest.fixture(scope="module")
def large_tile_case():
    """The oracle side of test_forward_at_a_size_where_the_large_tile_products_run, computed once for all its variants (the CPU forward and
    autograd backward of 110 crystals are ~20 s each)."""
    hpd = dict(M.TINY, emb_atom=256, emb_edge=256, num_blocks=2)
    hp = M.GemNetHParams(**hpd)
    P = M.init_params(hp, seed=8, head_scale=0.5)
    na, frac, cell, a, t, g = _case([20] * 110, seed=21, cell_scale=5.5)
    taps = {}
    ref = M.gemnet_forward(P, hp, frac, cell, a, na, t, taps=taps)
    N, B = int(na.sum()), len(na)
    up, uc, ul = torch.randn(N, 3, generator=g), M.symmetric_noise(torch.randn(B, 3, 3, generator=g)), torch.randn(N, 101, generator=g)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    refg = M.gemnet_forward(Pg, hp, frac, cell, a, na, t)
    ((refg["pos"] * up).sum() + (refg["cell"] * uc).sum() + (refg["atomic_numbers"] * ul).sum()).backward()
    return dict(hpd=hpd, hp=hp, P=P, na=na, frac=frac, cell=cell, a=a, t=t, taps=taps, ref={k: v.detach() for k, v in ref.items()}, up=up, uc=uc, ul=ul,
                grads={k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in Pg.items()})


@pytest.mark.parametrize("planes,f16,lean", [(1, 0, 1), (4, 0, 1), (5, 0, 1), (1, 0, 0), (2, 0, 1), (3, 0, 1), (0, 1, 1), (0, 0, 1)],
                         ids=["pre-split-plane-sets", "pre-split-plane-sets-general-row-epilogue", "pre-split-plane-sets-persistent-lean-grid", "pre-split-plane-sets-both-formats",
                              "pre-split-plane-sets-lds-dma-256-tiles", "pre-split-plane-sets-forward-only", "fp32-operand-fp16-2plane",
                              "fp32-operand-bf16-3plane"])
def test_forward_at_a_size_where_the_large_tile_products_run(planes, f16, lean, large_tile_case):
    """110 crystals x 20 atoms at width 256 (>= 16k edges): the edge-level dense layers run on the pre-split plane-set kernel
    (default: operands split once where they are produced, scales from one-layer bounds on exact absmax values; inference keeps one
    format per edge-level tensor and folds the skip merges into the residual stacks -- `lean`, also run switched off) or on the
    fp32-operand kernel (three bf16 planes or two fp16 planes split on the fly); all against the oracle, outputs and per-block taps,
    the register-tile kernel's launches that only write a plane set through its lean epilogue (default) or its general one;
    the plane-set variants also through the backward (whose edge-level data gradients run on the plane-set kernel too, dZ written as a
    plane set by the activation-gradient pass -- `planes` = 3 keeps them on the fp32-operand kernel)."""
    from matinvent_amd import _lib
    c = large_tile_case
    hp, P, na, frac, cell, a, t, taps, ref = c["hp"], c["P"], c["na"], c["frac"], c["cell"], c["a"], c["t"], c["taps"], c["ref"]
    m = _module(c["hpd"], P)
    _lib.check(_lib.load().mi_debug_set_mg_f16(f16))
    _lib.check(_lib.load().mi_debug_set_mg_planes(3 if planes == 3 else 1 if planes else 0))
    _lib.check(_lib.load().mi_debug_set_mg_lean(lean))
    if planes == 4:   # the register-tile kernel's general row epilogue (LDS patch) for the launches that by default take its lean one
        _lib.load().mi_debug_set_rt_lean(0)
    if planes == 5:   # the value 2 (it once selected a persistent grid: equal on four chains, 1.7 % slower on one) is accepted and behaves as 1
        _lib.load().mi_debug_set_rt_lean(2)
    if planes == 2:   # every qualifying product (epilogue extensions included) on the 256 x 256 LDS-DMA kernel, whatever its row count
        _lib.check(_lib.load().mi_debug_set_planes_big(2, 1))   # (the other cases take the default route: the 128 x 256 register-tile
        _lib.check(_lib.load().mi_debug_set_planes_rt(0, 0))    #  kernel of csrc/edge_stage.hip for these products)
    try:
        gb = m.decoder.make_batch(na)
        E = gb.graph(frac, cell)["src"].shape[0]
        assert E * 2 >= 256 * 128, E   # (E / 128) x (256 / 128) output tiles: the large-tile branch
        with torch.no_grad():
            out = m.decoder(frac, cell, a, t, gb)
        for k in ("pos", "cell", "atomic_numbers"):
            _rel(out[k], ref[k], 2e-5, f"{k} (planes={planes} f16={f16} lean={lean})")
        for i in range(hp.num_blocks):   # (tensors a lean forward kept as plane sets only are rebuilt from them for the tap)
            for name in (f"x3_{i}", f"h{i + 1}", f"m{i + 1}"):
                _rel(gb.tap(name), taps[name].reshape(-1), 2e-5, f"{name} (planes={planes} f16={f16} lean={lean})")
        assert _lib.saturation_events(reset=True) == 0
        if planes:   # the training forward + backward through the same plane-set layers: parameter gradients vs the oracle's autograd
            up, uc, ul = c["up"], c["uc"], c["ul"]
            o2 = m.decoder(frac, cell, a, t, gb)
            ((o2["pos"] * up.cuda()).sum() + (o2["cell"] * uc.cuda()).sum() + (o2["atomic_numbers"] * ul.cuda()).sum()).backward()
            for k, (o, n, shape) in m.decoder.layout.items():
                _rel(m.decoder.theta.grad[o:o + n].view(shape), c["grads"][k], 5e-5, f"grad {k}")
    finally:
        _lib.check(_lib.load().mi_debug_set_mg_f16(0))
        _lib.check(_lib.load().mi_debug_set_mg_planes(1))
        _lib.check(_lib.load().mi_debug_set_mg_lean(1))
        _lib.check(_lib.load().mi_debug_set_planes_big(1, 65536))
        _lib.check(_lib.load().mi_debug_set_planes_rt(2, 0))
        _lib.load().mi_debug_set_rt_lean(1)


# ---- the network at the size the benchmark times it: GemNetHParams() defaults (512 / 512 / 64 / 16 / 16, 4 blocks, 42.7 M parameters),
# ---- 256 crystals x 20 atoms at physical density (~250 k edges) -- BASELINE configs[1]-[2] in their MatterGen-labelled form
BENCH_B, BENCH_N = 256, 20


def _bench_state(B, seed=3, n=BENCH_N):
    """bench.py's mid-chain state: cells near the density prior's limit mean (n / rho)^(1/3) I with symmetric noise, uniform positions."""
    g = torch.Generator().manual_seed(seed)
    mu = (n / 0.05771451654022283) ** (1 / 3)
    cell = mu * torch.eye(3)[None].repeat(B, 1, 1) + 0.3 * M.symmetric_noise(torch.randn(B, 3, 3, generator=g))
    N = B * n
    return dict(na=torch.full((B,), n, dtype=torch.long), frac=torch.rand(N, 3, generator=g), cell=cell,
                a=torch.randint(1, 101, (N,), generator=g), t=0.1 + 0.8 * torch.rand(B, generator=g), g=g)


@pytest.fixture(scope="module")
def bench_net():
    hp = M.GemNetHParams()
    P = M.init_params(hp, seed=0, head_scale=20.0)   # (bench.py's weights: heads scaled so that score x std is of order one)
    return hp, P, _module(dict(), P)


def test_benchmark_size_forward_is_reproducible_finite_and_inside_the_plane_format(bench_net):
    """(i) B = 256 x 20 atoms, default hyper-parameters: two evaluations give the same bits (fixed reduction orders, no float atomics),
    every output is finite, and no conversion to the two-plane fp16 format saturated."""
    from matinvent_amd import _lib
    hp, P, m = bench_net
    s = _bench_state(BENCH_B)
    gb = m.decoder.make_batch(s["na"])
    _lib.saturation_events(reset=True)
    with torch.no_grad():
        o1 = {k: v.clone() for k, v in m.decoder(s["frac"], s["cell"], s["a"], s["t"], gb).items()}
        E = int(gb.graph(s["frac"], s["cell"])["src"].shape[0])
        o2 = m.decoder(s["frac"], s["cell"], s["a"], s["t"], gb)
    assert E >= 200_000, E   # the 256 k-edge regime of the benchmark line
    for k in o1:
        assert bool(torch.isfinite(o1[k]).all()), k
        assert torch.equal(o1[k], o2[k]), f"{k}: not bit-reproducible"
    assert _lib.saturation_events(reset=True) == 0


def test_benchmark_size_crystals_inside_the_full_batch_vs_the_oracle(bench_net):
    """(ii) Eight crystals of the benchmark batch through oracle.gemnet_forward on their own, against the same crystals' outputs
    INSIDE the 256-crystal batch: crystals never interact, but the power-of-two scales of the plane sets come from batch-wide maxima,
    so this bounds the batch-composition dependence of the 22-bit format at the size every published figure is taken at.
    Tolerance 5e-5 of max|ref| per output (the small-case forward tests use 2e-5)."""
    hp, P, m = bench_net
    s = _bench_state(BENCH_B)
    with torch.no_grad():
        out = m.decoder(s["frac"], s["cell"], s["a"], s["t"], m.decoder.make_batch(s["na"]))
    for first in (0, 124, 248):   # first, middle and last eight crystals
        g0, g1, n0, n1 = first, first + 8, first * BENCH_N, (first + 8) * BENCH_N
        with torch.no_grad():
            ref = M.gemnet_forward(P, hp, s["frac"][n0:n1], s["cell"][g0:g1], s["a"][n0:n1], s["na"][g0:g1], s["t"][g0:g1])
        _rel(out["pos"][n0:n1], ref["pos"], 5e-5, f"pos, crystals {g0}..{g1} of the full batch")
        _rel(out["cell"][g0:g1], ref["cell"], 5e-5, f"cell, crystals {g0}..{g1} of the full batch")
        _rel(out["atomic_numbers"][n0:n1], ref["atomic_numbers"], 5e-5, f"logits, crystals {g0}..{g1} of the full batch")


def _drop_handles(m):
    """Free a module's cached batch handles (graph buffers + activation arenas: tens of GB each at the benchmark size)."""
    import gc
    m.__dict__.pop("_gb_cache", None)
    m.__dict__.pop("_gb_chain_cache", None)
    m.__dict__.pop("_last_chain_batches", None)   # (the handles of the last sample() call, kept for graph_status())
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_benchmark_size_crystal_groups_vs_the_unsplit_batch(bench_net):
    """(iii) Four groups of 64 crystals against the unsplit batch of 256 (the split `chains` makes; same Philox draws through global ids, same
    per-crystal step sizes).  What differs is the batch-wide maxima behind the plane-set scales, i.e. the rounding of the 22-bit format.
      (a) ONE EVALUATION: a 64-crystal group alone vs the same crystals inside the unsplit batch -- 2e-5 of max|output| per head (the
          composition dependence of the network itself; measured ~1e-6);
      (b) ONE PREDICTOR-CORRECTOR STEP (two evaluations + updates) at a late grid point, the groups sampled ONE AFTER THE OTHER (bit-
          reproducible): types identical, cells within 5e-3 of max|cell|, the MEDIAN atom within 1e-4 (wrapped).  The maximum over the 5120
          atoms is NOT bounded: with random-init weights (heads scaled so that score x std is of order one) the Langevin step size
          2 (snr |z| / |score|)^2 and the 50-nearest selection amplify a 1e-6 difference to O(0.1) for a few atoms (measured: 0.16 for the worst
          atom, 9e-4 of max|cell|) -- DESIGN 11 records the same for the oracle against itself under a 1e-6 perturbation;
      (c) CONCURRENT chains (`chains=4`, the sampler's automatic choice at this size): two runs give the same bits, and those of the groups
          sampled one after the other.  (Round 3 could only report this: one quarter-wave of the position head intermittently differed.
          The cause was a fault of packed-fp32 VALU instructions next to another stream's LDS + MFMA kernel, scripts/force_fwd_repro.hip;
          the library is built without those instructions, matinvent_amd/build.py)"""
    hp, P, m = bench_net
    s = _bench_state(BENCH_B)
    with torch.no_grad():
        full = {k: v.clone() for k, v in m.decoder(s["frac"], s["cell"], s["a"], s["t"], m.decoder.make_batch(s["na"])).items()}
        for g0 in (0, 128):
            g1, n0, n1 = g0 + 64, g0 * BENCH_N, (g0 + 64) * BENCH_N
            part = m.decoder(s["frac"][n0:n1], s["cell"][g0:g1], s["a"][n0:n1], s["t"][g0:g1], m.decoder.make_batch(s["na"][g0:g1]))
            _rel(part["pos"], full["pos"][n0:n1], 2e-5, f"pos, group {g0}..{g1} alone vs inside the batch")
            _rel(part["cell"], full["cell"][g0:g1], 2e-5, f"cell, group {g0}..{g1} alone vs inside the batch")
            _rel(part["atomic_numbers"], full["atomic_numbers"][n0:n1], 2e-5, f"logits, group {g0}..{g1} alone vs inside the batch")
    state = dict(pos=s["frac"].cuda(), cell=s["cell"].cuda(), atomic_numbers=s["a"].cuda())
    i0 = 900   # t ~ 0.1: late in the chain
    kw = dict(n_steps=1000, seed=5, i_start=i0, i_stop=i0 + 1)
    whole = m.sample(s["na"], state={k: v.clone() for k, v in state.items()}, chains=1, **kw)[1]
    cuts = [BENCH_B * k // 4 for k in range(5)]

    def groups():
        outs = []
        for k in range(4):
            n0, n1 = cuts[k] * BENCH_N, cuts[k + 1] * BENCH_N
            st = dict(pos=state["pos"][n0:n1].clone(), cell=state["cell"][cuts[k]:cuts[k + 1]].clone(), atomic_numbers=state["atomic_numbers"][n0:n1].clone())
            outs.append(m.sample(s["na"][cuts[k]:cuts[k + 1]], state=st, node_offset=n0, graph_offset=cuts[k], chains=1, **kw)[1])
        return {k: torch.cat([o[k] for o in outs]) for k in ("pos", "cell", "atomic_numbers")}

    def dist(a, b):
        d = (a["pos"] - b["pos"]).abs()
        d = torch.minimum(d, 1 - d).max(dim=1).values
        return float((a["cell"] - b["cell"]).abs().max()) / float(a["cell"].abs().max()), d, int((a["atomic_numbers"] != b["atomic_numbers"]).sum())

    g1, g2 = groups(), groups()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), f"{k}: the groups sampled one after the other are not reproducible"
    dc, d, nt = dist(whole, g1)
    print(f"MEASURED four groups (one after the other) vs unsplit after one step: cell {dc:.3e} of max|cell|; positions (wrapped) median "
          f"{float(d.median()):.3e}, 99th percentile {float(d.quantile(0.99)):.3e}, max {float(d.max()):.3e}; {nt} types differ")
    assert nt == 0 and dc <= 5e-3 and float(d.median()) <= 1e-4, (dc, float(d.median()), nt)
    c1 = m.sample(s["na"], state={k: v.clone() for k, v in state.items()}, chains=4, **kw)[1]
    c2 = m.sample(s["na"], state={k: v.clone() for k, v in state.items()}, chains=4, **kw)[1]
    _drop_handles(m)
    dcc, dd, ntc = dist(c1, c2)
    dcs, ds, nts = dist(c1, g1)
    print(f"MEASURED four CONCURRENT chains: run vs run cell {dcc:.3e}, worst atom {float(dd.max()):.3e}, atoms that differ {int((dd > 0).sum())}; "
          f"vs the groups one after the other cell {dcs:.3e}, worst atom {float(ds.max()):.3e}, atoms that differ {int((ds > 0).sum())}")
    assert all(bool(torch.isfinite(c1[k].float()).all()) for k in c1) and ntc == 0
    for k in ("pos", "cell", "atomic_numbers"):
        assert torch.equal(c1[k], c2[k]), f"{k}: two runs of four concurrent chains differ"
        assert torch.equal(c1[k], g1[k]), f"{k}: four concurrent chains differ from the same groups sampled one after the other"


def test_benchmark_size_concurrent_forwards_are_bit_reproducible(bench_net):
    """Four 64-crystal groups evaluated CONCURRENTLY (four host threads, four streams, one batch handle each) against the same four
    forwards run one after the other: every output bit-identical in each of 40 trials.  With packed-fp32 VALU instructions in the
    library's small kernels 14 % of such trials differed in one quarter-wave of the position head (round 3's open finding; the fault is
    reproduced without any library code by scripts/force_fwd_repro.hip); the library is built without them (matinvent_amd/build.py)."""
    import threading
    from matinvent_amd.streams import concurrent_streams
    hp, P, m = bench_net
    _drop_handles(m)   # (four inference arenas of 64 crystals at ~38 GB each follow)
    print("free / total device memory before the four handles:", [round(x / 2**30, 1) for x in torch.cuda.mem_get_info()])
    G, Bg = 4, 64
    groups = []
    for k in range(G):
        s = _bench_state(Bg, seed=10 + k)
        groups.append({kk: (v.cuda() if torch.is_tensor(v) else v) for kk, v in s.items() if kk != "g"})
    gbs = [m.decoder.make_batch(gr["na"].cpu()) for gr in groups]
    m.decoder.sync()

    def fwd(k):
        gr = groups[k]
        with torch.no_grad():   # (grad mode is thread-local: every worker thread needs its own)
            return {kk: v.clone() for kk, v in m.decoder(gr["frac"], gr["cell"], gr["a"], gr["t"], gbs[k]).items()}

    ref = [fwd(k) for k in range(G)]
    torch.cuda.synchronize()
    pool = concurrent_streams(G, m.device)
    cur = torch.cuda.current_stream()
    differing = []
    for trial in range(40):
        out, err = [None] * G, [None] * G
        ready = cur.record_event()

        def run(k):
            try:
                with torch.cuda.stream(pool[k]):
                    pool[k].wait_event(ready)
                    out[k] = fwd(k)
                    cur.wait_event(pool[k].record_event())
            except BaseException as e:
                err[k] = e
        th = [threading.Thread(target=run, args=(k,)) for k in range(G)]
        [t.start() for t in th]
        [t.join() for t in th]
        torch.cuda.synchronize()
        assert all(e is None for e in err), err
        differing += [(trial, k, kk) for k in range(G) for kk in ref[k] if not torch.equal(out[k][kk], ref[k][kk])]
    del gbs
    _drop_handles(m)
    assert not differing, f"{len(differing)} outputs of concurrent forwards differ from the sequential ones: {differing[:6]}"


def test_benchmark_size_fine_tune_window_vs_the_oracle(bench_net):
    """(iv) A two-timestep accumulation window of ft_step at 64 crystals x 20 atoms with the benchmark network (the route
    `bench.py --mode mg-ft` takes; pipeline/mat_invent.py:150-177 over models/mattergen/pl_module.py:55-102) + the Adam step, against the
    same loop over the oracle with torch autograd.  The oracle walks the set in chunks of 16 crystals (the update is a sum over
    crystals; this only bounds its memory)."""
    from matinvent_amd.finetune import ft_step
    from matinvent_amd.mattergen import ChemGraph, symmetrize_lattice
    hp, _, m_fix = bench_net
    _drop_handles(m_fix)   # (the training arenas of 64 crystals are ~43 GB each: agent forward, its gradient mirror, the prior)
    B, TS = 64, 2
    P0, Q0 = M.init_params(hp, seed=0, head_scale=0.3), M.init_params(hp, seed=0, head_scale=0.3)
    g = torch.Generator().manual_seed(31)
    for k in P0:
        P0[k] = P0[k] + 0.01 * torch.randn(P0[k].shape, generator=g)
    agent, prior = _module(dict(), P0), _module(dict(), Q0)
    prior.requires_grad_(False)
    s = _bench_state(B, seed=41)
    na, frac, cell, a = s["na"], s["frac"], s["cell"], s["a"]
    N = int(na.sum())
    off = [0] + torch.cumsum(na, 0).tolist()
    data = [ChemGraph(frac[off[i]:off[i + 1]], cell[i:i + 1], a[off[i]:off[i + 1]]) for i in range(B)]
    rewards = torch.rand(B, generator=g).numpy()
    noises = {(0, t): (torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g), torch.rand(N, generator=g)) for t in range(TS)}
    cfg = dict(lr=1e-5, accum_steps=TS, epochs=1, timesteps=TS, sigma=0.025)   # (lr of configs/model/mattergen.yaml:13)
    stats = ft_step(agent, prior, data, rewards, cfg, noise_fn=lambda e, t: noises[(e, t)])
    corr = M.Corruption()
    rw = torch.from_numpy(rewards).float()
    A = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    grads = {k: torch.zeros_like(v) for k, v in A.items()}
    tot = 0.0
    CH = 16
    for ti in range(TS):
        for c0 in range(0, B, CH):
            c1, n0, n1 = c0 + CH, off[c0], off[c0 + CH]
            ob = dict(pos=frac[n0:n1], cell=symmetrize_lattice(cell[c0:c1]), atomic_numbers=a[n0:n1], num_atoms=na[c0:c1])
            t = torch.full((CH,), M.time_grid(corr, ti))
            nz = noises[(0, ti)]
            noisy, aux = M.sample_marginal(corr, ob, t, dict(pos=nz[0][n0:n1], cell=nz[1][c0:c1], types=nz[2][n0:n1]))
            pa = M.gemnet_forward(A, hp, noisy["pos"], noisy["cell"], noisy["atomic_numbers"], na[c0:c1], t)
            with torch.no_grad():
                pp = M.gemnet_forward(Q0, hp, noisy["pos"], noisy["cell"], noisy["atomic_numbers"], na[c0:c1], t)
            sl, _ = M.sample_loss(corr, ob, aux, pa)
            kl = M.calc_kl_reg(pa, pp, aux["node2graph"], CH)
            loss = (rw[c0:c1] * sl + 0.025 * kl * (1.1 - rw[c0:c1])).sum() / (B * TS)
            gs = M.param_grads(loss, A)
            for k, gg in zip(A, gs):
                grads[k] += gg
            tot += float(loss.detach()) * TS
            del pa, pp, sl, kl, loss, gs
    # (2e-3, not the forward's 2e-5: the device noises the structures itself, and its noised positions differ from the oracle's in the last bit
    #  (`% 1.0` of a sum, 2e-6 allowed by test_add_noise_...).  128 radial Gaussians 0.055 A wide turn 7e-6 A into 1e-4 of a basis value, and this
    #  randomly perturbed 42.7 M-parameter network (outputs of order 1e4) into up to 1 % of ONE crystal's loss -- measured with identical edge
    #  lists on both sides, scripts/mg_loss_check.py: 8e-5 / 2.6e-4 of the summed sample loss, 4e-4 / 1e-3 of the KL term at the two timesteps.
    #  On IDENTICAL inputs the same network agrees to 1e-5 per output: scripts/mg_scale_check.py and tests (i)-(iii).)
    assert abs(stats[0]["loss"] - tot / TS) <= 2e-3 * max(1.0, abs(tot / TS)), (stats[0]["loss"], tot / TS)
    with torch.no_grad():
        Ad = {k: v.detach().clone() for k, v in A.items()}
        DO.adam_step(Ad, grads, {}, 1e-5)
    bad = tot_n = 0
    for k, w in agent.decoder.views().items():
        d = (w.detach().cpu() - Ad[k]).abs()
        assert float(d.max()) <= 2.1e-5, f"{k}: {float(d.max())}"   # (an Adam step moves a weight by at most ~lr = 1e-5)
        bad += int((d > 1e-6).sum())
        tot_n += d.numel()
    assert bad <= 0.02 * tot_n, f"{bad} of {tot_n} parameters differ by more than 1e-6 after the Adam step"


def test_adapter_arithmetic_on_the_device_against_the_reference_generated_fixture():
    """The product adapter (matinvent_amd/mattergen.py, tensors on the GPU) against tests/golden/g12_mattergen_adapter.npz -- outputs of the reference's own
    pl_module.py / loss.py (tests/golden/make_golden.py::g12_mattergen_adapter): anchor penalty on a ragged batch, the time grid add_noise hands the corruption,
    the default loss weights and the weighted stack-sum.  Row a17 reads "adapter arithmetic pinned, network unpinned"."""
    import os
    from matinvent_amd import mattergen as MG
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_mattergen_adapter.npz"))
    dev = torch.device("cuda", 0)
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    m = _module(M.TINY)
    na = torch.from_numpy(g["kl_num_atoms"])
    n2g = torch.repeat_interleave(torch.arange(len(na)), na)

    class Batch:
        num_atoms = na

        def get_batch_idx(self, key):
            return n2g

    agent = dict(pos=t("kl_agent_pos"), cell=t("kl_agent_cell"), atomic_numbers=t("kl_agent_types"))
    prior = dict(pos=t("kl_prior_pos"), cell=t("kl_prior_cell"), atomic_numbers=t("kl_prior_types"))
    kl = m.calc_kl_reg(agent, prior, Batch())
    assert kl.is_cuda
    _rel(kl, g["kl_out"], 2e-6, "anchor penalty vs the reference's calc_kl_reg")
    # add_noise's t (every crystal gets linspace(T_max, 1/1000, 1000)[timestep]): bit-equal float32
    gen = torch.Generator().manual_seed(3)
    N, B = int(na.sum()), len(na)
    cell = 6.0 * torch.eye(3)[None].repeat(B, 1, 1)
    batch = _batch_obj(na, torch.rand(N, 3, generator=gen), cell, torch.randint(1, 101, (N,), generator=gen))
    for tmax, key in ((1.0, "grid_t_Tmax1p0"), (0.8, "grid_t_Tmax0p8")):
        m.T = tmax
        for k, want in zip(g["grid_timesteps"], g[key]):
            _, _, tt = m.add_noise(batch, int(k))
            assert tt.is_cuda and tt.shape == (B,) and np.array_equal(tt.cpu().numpy(), np.full(B, want, dtype=np.float32)), (tmax, k)
    # SampleLoss: weights and aggregation
    assert [MG.WEIGHTS[k] for k in g["loss_fields"]] == list(g["loss_weights"]) and MG.D3PM_LAMBDA == float(g["loss_d3pm_hybrid_lambda"])
    fields = dict(pos=t("loss_pos"), cell=t("loss_cell"), atomic_numbers=t("loss_types"))
    assert torch.equal(MG.weighted_field_sum(fields).cpu(), torch.from_numpy(g["loss_agg"]))
    assert torch.equal(MG.weighted_field_sum(fields, dict(zip(g["loss_fields"], g["loss_weights_custom"]))).cpu(), torch.from_numpy(g["loss_agg_custom"]))
