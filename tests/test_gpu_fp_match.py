"""GPU checks of fingerprint matching (matinvent_amd/csrc/fp_match.hip, include/matinvent_hip_match.h, matinvent_amd.novelty)
against the float64 restatement tests/fp_match_ref.py:

1. distances at the sizes the loops turn over (ncols 1 .. 2304, 0 .. 257 candidates, 1 .. 9 queries per group, one call, pair matrix on);
2. both ends of the work-item builder: 300 groups of 1 x 1, and one group of 64 x 1200 without the pair matrix;
3. bit reproducibility of one pair: call to call, list reversed, groups permuted, alone, inside the large group;
4. ties to the lowest bank index, whatever the order of the list;
5. real fingerprints: novel_mask / unique_mask on crystals, their copies and re-descriptions;
6. UNFilter end to end: the sampler's output twice, a drop-in MatInvent loop and a fixed-formula MatInventDPO loop;
7. the C entry's refusals.

Error budget of (1), per pair: |d_dev - d_64| <= (L(ncols) + 8) 2^-24 1/2 sum |u_i v_i| + 2^-24 with L the chain length the header states
(4 ceil(ceil4(ncols) / 256) + 6): the standard bound of a floating-point sum of that depth -- the products are exact inside the FMAs --
plus one rounding each for the subtraction, the halving and the store.  It comes from the kernel's documented order, not from a run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, novelty, structure
from matinvent_amd.structure import FP_TOL
from tests import fp_match_ref as R
from tests import fp_ref64

pytestmark = pytest.mark.gpu
DEV = "cuda"
CSR = ("grp_q_off", "q_idx", "grp_c_off", "c_idx", "grp_ncols")


def _bank(rows):
    bank = novelty.FingerprintBank(device=DEV)
    got = bank.add_rows([f"len{len(r)}" for r in rows], [len(r) for r in rows], list(rows), np.zeros(len(rows), np.int64))
    assert got == list(range(len(rows)))
    return bank


def _call(query, groups, bank, tol, pairs=True, chunk=0):
    packed = R.pack(groups, [])
    out = novelty._run_kernel(query, {k: packed[k] for k in CSR}, bank, tol, pairs, chunk)
    torch.cuda.synchronize()
    return out


def test_distances_against_float64_at_the_sizes_the_loops_turn_over():
    case = R.distance_case()
    bank = _bank(case["bank_rows"])
    bd, bi, nw, st, mats = _call(case["query"], case["groups"], bank, R.TOL)
    worst = R.check_distances(case, bd, bi, nw, st, mats, R.TOL, "device")
    assert set(worst) == set(R.NCOLS)
    empty = [g for g in case["groups"] if not g[1]]
    assert len(empty) == len(R.NCOLS) * len(R.NQUERY)
    for q_rows, _, _ in empty:
        assert (bi[q_rows] == -1).all() and (nw[q_rows] == 0).all() and (st[q_rows] == 0).all()


@pytest.fixture(scope="module")
def wide():
    """300 groups of 1 x 1 and one group of 64 x 1200, ncols = 192: rows, groups, the float64 answers -- computed once."""
    rows = list(R.unit_rows(300 + 1200, 192, 192, 5))
    query = R.unit_rows(300 + 64, 192, 192, 6)
    groups = [([k], [k], 192) for k in range(300)] + [(list(range(300, 364)), list(range(300, 1500)), 192)]
    want = R.match_groups(query, groups, rows, [192] * 1500, 0.3)
    return dict(rows=rows, query=query, groups=groups, want=want, bank=_bank(rows))


def test_many_small_groups_and_one_large_group(wide):
    bd, bi, nw, st, mats = _call(wide["query"], wide["groups"], wide["bank"], 0.3, pairs=False)
    want_d, want_i, want_n, _, want_pairs = wide["want"]
    assert mats is None and not st.any()
    assert (bi == want_i).all() and (nw == want_n).all()
    for (q_rows, c_rows, ncols), d64 in zip(wide["groups"], want_pairs):
        for j, q in enumerate(q_rows):
            assert abs(float(bd[q]) - d64[j].min()) <= R.budget(wide["query"][q], wide["rows"][int(bi[q])], ncols)


def test_one_pair_has_the_same_bits_wherever_it_is_computed(wide):
    query, groups, bank = wide["query"], wide["groups"], wide["bank"]
    a = _call(query, groups, bank, 0.3)
    b = _call(query, groups, bank, 0.3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4])) and a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()
    big = a[4][300]
    rev = _call(query, groups[:300] + [(groups[300][0], groups[300][1][::-1], 192)], bank, 0.3)
    assert rev[4][300][:, ::-1].tobytes() == big.tobytes() and rev[0].tobytes() == a[0].tobytes() and (rev[1] == a[1]).all()
    perm = np.random.default_rng(0).permutation(301)
    shuffled = _call(query, [groups[k] for k in perm], bank, 0.3, chunk=48)        # and another cut into chunks
    for pos, k in enumerate(perm):
        assert shuffled[4][pos].tobytes() == a[4][k].tobytes()
    assert shuffled[0].tobytes() == a[0].tobytes() and (shuffled[1] == a[1]).all() and (shuffled[2] == a[2]).all()
    for qi, ci in ((0, 0), (9, 1199), (63, 517), (31, 16)):
        alone = _call(query, [([300 + qi], [300 + ci], 192)], bank, 0.3)
        assert alone[4][0].tobytes() == big[qi:qi + 1, ci:ci + 1].tobytes()
        assert alone[0][300 + qi].tobytes() == big[qi, ci].tobytes() and alone[1][300 + qi] == 300 + ci


def test_ties_resolve_to_the_lowest_bank_index():
    rows = list(R.unit_rows(9, 64, 64, 11))
    rows[5] = rows[2].copy()
    rows[7] = rows[2].copy()
    bank = _bank(rows)
    q = rows[2].astype(np.float64) + 0.05 * R.unit_rows(1, 64, 64, 12)[0]
    query = np.stack([(q / np.linalg.norm(q)).astype(np.float32), rows[4]])
    for order in ([7, 2, 5], [5, 7, 2]):
        bd, bi, nw, st, mats = _call(query, [([0], order, 64)], bank, 0.02)
        assert bi[0] == 2 and mats[0][0, 0] == mats[0][0, 1] == mats[0][0, 2] == bd[0] and nw[0] in (0, 3) and st[0] == 0
    bd, bi, nw, st, mats = _call(query, [([0], [8, 7, 6, 5, 4, 3, 2, 1, 0], 64)], bank, 0.02)
    assert bi[0] == 2
    bd, bi, nw, st, _ = _call(query, [([1], list(range(9)), 64)], bank, 0.02)      # a query equal to a bank row
    assert bi[1] == 4 and nw[1] >= 1 and abs(float(bd[1])) <= R.budget(rows[4], rows[4], 64)


# ---- real fingerprints ----------------------------------------------------------------------------------------------------------------------
RATTLE_SEED = 0


def _crystals():
    from tests.test_gpu_fingerprint import _struc
    a, b = fp_ref64.rock_salt(), fp_ref64.cscl_type()
    c = fp_ref64.random_crystal(6, [3, 8], 1)
    d = (c[0], fp_ref64.random_crystal(6, [3, 8], 2)[1], c[2])                      # independently drawn coordinates of one composition
    g = np.random.default_rng(RATTLE_SEED)
    copy = (a[0], a[1] + g.normal(0, 0.02 / np.sqrt(3), a[1].shape) @ np.linalg.inv(a[2]), a[2])   # |displacement| ~ 0.02 A
    redesc = fp_ref64.translated(fp_ref64.permuted(d))
    third = fp_ref64.random_crystal(5, [26], 3)
    other = (a[0], fp_ref64.random_crystal(8, [11, 17], 3)[1], a[2])               # a distinct structure of a banked formula
    raw = dict(a=a, b=b, c=c, d=d, copy=copy, redesc=redesc, third=third, other=other, a2=fp_ref64.permuted(a))
    return raw, {k: _struc(v) for k, v in raw.items()}


def test_masks_on_real_fingerprints():
    raw, s = _crystals()
    u = {k: fp_ref64.fingerprint(*v)["u"] for k, v in raw.items() if k in ("a", "b", "copy", "other")}
    d_copy = fp_ref64.distance(u["a"], u["copy"])
    print(f"d(rock salt, rattled copy) = {d_copy:.3g}; d(rock salt, other) = {fp_ref64.distance(u['a'], u['other']):.3g}")
    assert d_copy < FP_TOL / 2                                                        # a margin of 2
    assert min(fp_ref64.distance(u["other"], u["a"]), fp_ref64.distance(u["other"], u["b"]), fp_ref64.distance(u["a"], u["b"])) > 2 * FP_TOL
    banked = [s["a"], s["b"], s["c"], s["d"]]
    bank = novelty.FingerprintBank.from_records(banked)
    assert len(bank) == 4 and len(bank.formulas) == 2
    probe = [s["copy"], s["redesc"], s["third"], s["other"]]
    novel = novelty.novel_mask(probe, bank)
    assert novel.tolist() == [False, False, True, True]
    bd, bi, nw = novelty.match(probe, bank)
    assert bi.tolist()[:3] == [0, 3, -1] and nw.tolist()[:3] == [1, 1, 0] and bd[0] <= FP_TOL and np.isinf(bd[2])
    batch = [s["a"], s["copy"], s["b"], s["a2"]]
    unique = novelty.unique_mask(batch)
    assert unique.tolist() == [True, False, True, False]
    # both masks from the restatement, on the device's own rows
    fp_b, st_b = structure.record_fingerprints(banked)
    fp_p, st_p = structure.record_fingerprints(probe)
    fp_u, st_u = structure.record_fingerprints(batch)
    f = lambda recs: [structure.reduced_formula(r.species) for r in recs]
    assert R.novel_mask(f(probe), fp_p, st_p, f(banked), fp_b, st_b, FP_TOL).tolist() == novel.tolist()
    assert R.unique_mask(f(batch), fp_u, st_u, FP_TOL).tolist() == unique.tolist()


def test_unfilter_on_the_samplers_output():
    import tests.test_gpu_respaced_chain as RC
    from matinvent_amd.sampling import DiffCSPSampler
    base, _ = RC._base()
    flt = novelty.UNFilter(remember=True)
    np.random.seed(0)                                                   # (the atom counts come from numpy's global generator)
    data, strucs = DiffCSPSampler(seed=5).generate(base, batch_size=8, num_batches=1)
    want = novelty.unique_mask(strucs)
    kept_data, kept, m = flt(data, strucs, None)
    assert kept == [x for x, k in zip(strucs, want) if k] and kept_data == [x for x, k in zip(data, want) if k] and len(kept) >= 1
    assert m["novel_frac"] == 1.0 and m["unique_frac"] == want.mean() == m["un_frac"] and m["bank_size"] + sum(flt.bank.flagged.values()) == float(want.sum())
    np.random.seed(0)
    data2, strucs2 = DiffCSPSampler(seed=5).generate(base, batch_size=8, num_batches=1)
    assert [x.species for x in strucs2] == [x.species for x in strucs]
    kept_data2, kept2, m2 = flt(data2, strucs2, None)
    assert kept2 == [] and kept_data2 == [] and m2["novel_frac"] == 0.0 and m2["bank_size"] == m["bank_size"]


KEYS = ("unique_frac", "novel_frac", "un_frac", "bank_size")


@pytest.mark.parametrize("pipeline", ["mat_invent", "mat_invent_dpo"])
def test_dropin_loop_with_the_filter_from_the_config_front_end(tmp_path, monkeypatch, pipeline):
    """One drop-in loop with sample_cfg.filter composed from configs/filter/un.yaml; under MatInventDPO with a fixed formula, the
    single-formula case.  The untrained network's cells are given physical volumes first (tests/test_gpu_fingerprint.py explains why)."""
    import csv
    from matinvent_amd.data import data2struc
    from matinvent_amd.sampling import DiffCSPSampler
    from tests.test_gpu_fingerprint import FT, _dense, _dropin
    real_gen = DiffCSPSampler.generate

    def gen(self, *a, **kw):
        data, _ = real_gen(self, *a, **kw)
        data = [_dense(d) for d in data]
        return data, [data2struc(d) for d in data]

    monkeypatch.setattr(DiffCSPSampler, "generate", gen)
    args = ["expname=un", "+filter@sample_cfg.filter=un", "+sample_cfg.filter.fp_args={r_max: 3.0, sigma: 0.1}"] + FT
    if pipeline == "mat_invent_dpo":
        args += ["pipeline=mat_invent_dpo", "pipeline.finetune_cfg.timesteps=6", "pipeline.finetune_cfg.dpo_beta=1.0", "reward.mode=uniform",
                 "+sample_cfg.target_compositions_dict=[{Li: 2, O: 1}]"]
    rl = _dropin(tmp_path, args, 1)
    flt = rl.sample_cfg.filter
    assert isinstance(flt, novelty.UNFilter) and flt.remember and flt.fp_args == {"r_max": 3.0, "sigma": 0.1}
    rows = list(csv.DictReader(open(tmp_path / "exp_res" / "un" / "metrics.csv")))
    assert len(rows) == 1
    for k in KEYS:
        assert k in rows[0] and np.isfinite(float(rows[0][k])), k
    assert float(rows[0]["novel_frac"]) == 1.0 and 0 < float(rows[0]["un_frac"]) <= 1.0
    assert float(rows[0]["bank_size"]) + sum(flt.bank.flagged.values()) == rl.cost == len(rl.ltm)   # what passed is what was scored
    if pipeline == "mat_invent_dpo":
        assert flt.bank.formulas == ["Li2O"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_the_c_entry_refuses_bad_arguments_before_anything_is_enqueued():
    lib = _lib.load()
    rows = list(R.unit_rows(3, 8, 8, 1))
    bank = _bank(rows)
    q = torch.from_numpy(R.unit_rows(2, 8, 8, 2)).to(DEV)
    ints = torch.tensor([0, 2, 0, 1, 0, 3, 0, 1, 2, 8, 0, 0, 0, 3, 0, 0, 8], dtype=torch.int32, device=DEV)   # offsets, indices, one item, part offsets
    out = torch.full((8,), 7, dtype=torch.int32, device=DEV)
    work = torch.zeros(64, dtype=torch.int32, device=DEV)
    at = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)

    def args(**kw):
        a = _lib.FpMatchArgs()
        a.query, a.bank, a.bank_start, a.bank_len = at(q), at(bank.rows), at(bank.start), at(bank.length)
        a.grp_q_off, a.q_idx, a.grp_c_off, a.c_idx, a.grp_ncols, a.items, a.grp_part_off = at(ints), at(ints, 2), at(ints, 4), at(ints, 6), at(ints, 9), at(ints, 10), at(ints, 15)
        a.workspace, a.best_dist, a.best_idx, a.n_within, a.status = at(work), at(out), at(out, 2), at(out, 4), at(out, 6)
        a.bank_floats, a.pair_floats, a.Q, a.row_stride, a.M, a.G, a.nnz_q, a.nnz_c, a.n_items, a.n_partials, a.max_ncols, a.tol = 24, 0, 2, 8, 3, 1, 2, 3, 1, 8, 8, 0.02
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, text in ((dict(tol=1.5), "tol"), (dict(tol=float("nan")), "tol"), (dict(row_stride=6), "row_stride"), (dict(best_idx=None), "null output"),
                     (dict(bank=None), "null input"), (dict(Q=-1), "negative")):
        rc = lib.mi_fp_match(C.byref(args(**kw)), stream)
        assert rc == _lib.MI_EINVAL and text in lib.mi_last_error().decode(), (kw, lib.mi_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                       # nothing ran
    assert lib.mi_fp_match(C.byref(args(G=0)), stream) == 0 and lib.mi_fp_match(C.byref(args(Q=0)), stream) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert lib.mi_fp_match(C.byref(args()), stream) == 0               # and the same block, untouched, is a valid call
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    want = R.match_groups(q.cpu().numpy(), [([0, 1], [0, 1, 2], 8)], rows, [8, 8, 8], 0.02)
    assert host[2:4].tolist() == want[1].tolist() and host[4:6].tolist() == want[2].tolist() and host[6:8].tolist() == [0, 0]
    assert np.abs(host[:2].view(np.float32) - want[0]).max() < 1e-6
    # an item that does not lie inside its group (its candidates end past the group's) is rejected as a whole: nothing is read, no partial
    # is written, and both queries say so -- whatever the workspace held before
    bad = ints.clone()
    bad[13] = 4
    work.fill_(12345)
    assert lib.mi_fp_match(C.byref(args(items=at(bad, 10))), stream) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[2:4].tolist() == [-1, -1] and host[4:6].tolist() == [0, 0] and host[6:8].tolist() == [1, 1] and np.isinf(host[:2].view(np.float32)).all()
    assert lib.mi_fp_match_workspace(-1) == _lib.MI_EINVAL and lib.mi_fp_match_workspace(8) >= 8 * 16
