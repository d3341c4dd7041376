"""Reference arithmetic of classifier guidance (include/matinvent_hip_inputgrad.h): the property predictor's INPUT gradient by
torch.autograd on tests/scalar_ref.forward in float32 and float64, a central finite difference of the same forward, the seed of
mi_guide_seed and the shift of mi_guide_shift in float64 (and the float32 formulas, for the deviation a bound is taken from).  Plain
torch / numpy, CPU; a helper, not a test."""
import numpy as np
import torch

from tests import scalar_ref as SR

MODE_MAX, MODE_MIN, MODE_TARGET = 0, 1, 2


def input_grad(P, hp, t_emb, onehot, frac, lattices, num_atoms, d_out, dtype=torch.float32, wrap=True):
    """-> (out [B, P], g_frac [N, 3], g_lat [B, 3, 3], g_types [N, 100]) in `dtype`: the gradient of sum_bp d_out[b][p] out[b][p] -- the
    crystals are independent, so row b is the gradient of crystal b's own term."""
    c = lambda v: torch.as_tensor(v).to(dtype)
    ty, fr, lt = (c(v).detach().clone().requires_grad_(True) for v in (onehot, frac, lattices))
    out, _, _ = SR.forward(P, hp, c(t_emb), ty, fr, lt, num_atoms, dtype)
    g = torch.autograd.grad((out * c(d_out)).sum(), [fr, lt, ty])
    return out.detach(), g[0], g[1], g[2]


def finite_difference(P, hp, t_emb, onehot, frac, lattices, num_atoms, d_out, which, index, h=1e-6):
    """Central difference in float64 of sum_bp d_out out with respect to element `index` (a tuple) of `which` in ("frac", "lat", "types")."""
    dt = torch.float64
    c = lambda v: torch.as_tensor(v).to(dt).clone()
    vals = []
    for sgn in (+1.0, -1.0):
        arr = dict(types=c(onehot), frac=c(frac), lat=c(lattices))
        arr[which][index] += sgn * h
        out, _, _ = SR.forward(P, hp, c(t_emb), arr["types"], arr["frac"], arr["lat"], num_atoms, dt)
        vals.append(float((out * c(d_out)).sum()))
    return (vals[0] - vals[1]) / (2 * h)


def seed(out, p, mode, target_hat):
    """mi_guide_seed: float32 in, float32 out (the three formulas are exact or one rounded subtraction)."""
    out = np.asarray(out, dtype=np.float32)
    d = np.zeros_like(out)
    o = out[:, p]
    ok = np.isfinite(o)
    with np.errstate(invalid="ignore"):
        v = np.float32(1.0) if mode == MODE_MAX else (np.float32(-1.0) if mode == MODE_MIN else -(o - np.float32(target_hat)))
    d[:, p] = np.where(ok, v, np.float32(0.0))
    return d


def shift(types, frac, lat, g_types, g_frac, g_lat, num_atoms, a_t, a_x, a_l, max_shift, dtype=np.float64):
    """mi_guide_shift in `dtype`: state + clamp(a g), coordinates % 1; a crystal with a non-finite gradient element keeps its rows (the
    input's bits).  Returns (types, frac, lat, shifted [B] bool)."""
    f = lambda v: None if v is None else np.asarray(v.cpu() if torch.is_tensor(v) else v)
    types, frac, lat, g_types, g_frac, g_lat = (f(v) for v in (types, frac, lat, g_types, g_frac, g_lat))
    na = [int(v) for v in num_atoms]
    off = np.concatenate([[0], np.cumsum(na)])
    B = len(na)
    lat, g_lat = lat.reshape(B, 9), g_lat.reshape(B, 9)
    ot, ox, ol = types.astype(dtype).copy(), frac.astype(dtype).copy(), lat.astype(dtype).copy()
    done = np.zeros(B, dtype=bool)

    def step(a, g):
        v = dtype(a) * g.astype(dtype)
        return np.clip(v, -dtype(max_shift), dtype(max_shift)) if max_shift > 0 else v

    for b in range(B):
        r = slice(off[b], off[b + 1])
        ok = np.isfinite(g_lat[b]).all() and np.isfinite(g_frac[r]).all() and (g_types is None or np.isfinite(g_types[r]).all())
        if not ok:
            continue
        done[b] = True
        ol[b] = ol[b] + step(a_l, g_lat[b])
        ox[r] = np.mod(ox[r] + step(a_x, g_frac[r]), dtype(1.0))
        if g_types is not None:
            ot[r] = ot[r] + step(a_t, g_types[r])
    return ot, ox, ol.reshape(B, 3, 3), done
