"""One launch of Adam (adam_body of csrc/cwn_norm.hip, behind cwn_adam_f32 and cwn_adam_dev_f32) as a float64 reference that
carries its error bound (tests/_bounds.Tracked), the same formula in numpy float32 (the restatement of gate (E)), the wrong
variants the gates must refuse, and the graded operands all of them run on.  Shared by tests/test_bounds_host.py (CPU: the
gates pass the restatement and refuse every variant) and tests/test_gpu_adam_componentwise.py (the kernels).

    gr = g + wd p;  m' = b1 m + (1 - b1) gr;  v' = b2 v + (1 - b2) gr gr
    p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

The hyperparameters enter at their float32 values: what the kernel arguments and the device record hold."""
import numpy as np
import torch

from tests import _bounds as B

LR, EPS = 1e-3, 1e-8
HYPERS = [(0.9, 0.999, 0.0), (0.9, 0.999, 0.01), (0.8, 0.99, 0.01)]          # beta1, beta2, weight decay
HYPER_IDS = ['b.9-.999-wd0', 'b.9-.999-wd.01', 'b.8-.99-wd.01']
STEPS = (1, 2, 3, 10, 1000, 100000)
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)       # a thread owns four elements, a workgroup 1024
ALTERED = ('eps_in_root', 'eps_over_bc2', 'decoupled_wd', 'bias_at_t_minus_1', 'tail_unwritten')


def f32(x) -> float:
    return float(np.float32(x))


def _graded(n, gen, step, period, low, first):
    """sign * mantissa in [1, 2) * 2^e, e walking [-low, period - low) with stride `step` from element `first` on."""
    e = ((torch.arange(n) + first) * step) % period - low
    mant = 1 + torch.rand(n, generator=gen)
    sign = torch.randint(0, 2, (n,), generator=gen) * 2.0 - 1
    return (sign * torch.ldexp(mant, e)).float()


def operands(n: int, hyper, seed: int = 0):
    """(p, g, m, v) float32 CPU tensors [n]: |g| over 2^-40 .. 2^10 (sqrt(v') from far below eps to far above it), |p| over
    2^-20 .. 1, m and v the moments a first step leaves behind on ANOTHER graded gradient with signs of its own (so b1 m and
    (1 - b1) gr disagree in sign on about half of the elements, at every ratio of magnitudes).  Everything is normal in float32:
    the smallest product, (1 - b2) g g, is about 2^-90."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    b1, b2, _ = (np.float32(h) for h in hyper)
    g = _graded(n, gen, 7, 50, 40, n)
    p = _graded(n, gen, 3, 20, 20, n)
    g_prev = _graded(n, gen, 11, 50, 40, 3 * n + 1).numpy()
    m = (np.float32(1) - b1) * g_prev
    v = (np.float32(1) - b2) * g_prev * g_prev
    return p, g, torch.from_numpy(m), torch.from_numpy(v)


def reference(p, g, m, v, t: int, hyper, lr: float = LR, eps: float = EPS):
    """(m', v', p') as Tracked.  1 - beta is exact in float32 (beta in [1/2, 1]); with wd = 0 the kernel's g + 0 p is g."""
    b1, b2, wd = (f32(h) for h in hyper)
    P, G, M, V = B.inp(p), B.inp(g), B.inp(m), B.inp(v)
    gr = G if wd == 0.0 else B.add(G, B.mul(B.scalar(wd), P))
    m1 = B.add(B.mul(B.scalar(b1), M), B.mul(B.scalar(1 - b1), gr))
    v1 = B.add(B.mul(B.scalar(b2), V), B.mul(B.mul(B.scalar(1 - b2), gr), gr))
    bc1 = B.sub(B.scalar(1), B.power(B.scalar(b1), float(t)))
    bc2_sqrt = B.sqrt(B.sub(B.scalar(1), B.power(B.scalar(b2), float(t))))
    denom = B.add(B.div(B.sqrt(v1), bc2_sqrt), B.scalar(f32(eps)))
    p1 = B.sub(P, B.mul(B.div(B.scalar(f32(lr)), bc1), B.div(m1, denom)))
    return m1, v1, p1


def restatement(p, g, m, v, t: int, hyper, lr: float = LR, eps: float = EPS, alter=None):
    """(m', v', p') in numpy float32, in the kernel's order of operations -- or one of ALTERED."""
    f = np.float32
    p, g, m, v = (x.numpy().astype(f) for x in (p, g, m, v))
    b1, b2, wd, lr, eps = f(hyper[0]), f(hyper[1]), f(hyper[2]), f(lr), f(eps)
    tt = f(t - 1 if alter == 'bias_at_t_minus_1' else t)
    bc1, bc2_sqrt = f(1) - np.power(b1, tt), np.sqrt(f(1) - np.power(b2, tt))
    step_size = lr / bc1
    p_in = p
    if alter == 'decoupled_wd':                  # AdamW: the decay shrinks the parameter and stays out of the moments
        gr, p_in = g, p * (f(1) - lr * wd)
    else:
        gr = g + wd * p
    m1 = b1 * m + (f(1) - b1) * gr
    v1 = b2 * v + (f(1) - b2) * gr * gr
    if alter == 'eps_in_root':
        denom = np.sqrt(v1 + eps) / bc2_sqrt
    elif alter == 'eps_over_bc2':
        denom = (np.sqrt(v1) + eps) / bc2_sqrt
    else:
        denom = np.sqrt(v1) / bc2_sqrt + eps
    p1 = p_in - step_size * (m1 / denom)
    if alter == 'tail_unwritten' and p.size % 4:
        m1[-1], v1[-1], p1[-1] = m[-1], v[-1], p[-1]
    assert m1.dtype == v1.dtype == p1.dtype == f
    return torch.from_numpy(m1), torch.from_numpy(v1), torch.from_numpy(p1)


def judge(got, ref, cpu32, what: str):
    """The figures of one launch: (R) ratios of m' and v', the (E) ratio of p', its limit and the restatement's ratio.
    got / cpu32: (m', v', p'); ref: reference()."""
    rm = B.ratio(got[0], ref[0], what + " m' (R)")
    rv = B.ratio(got[1], ref[1], what + " v' (R)")
    rc = B.ratio(cpu32[2], ref[2], what + " p' float32 numpy on the CPU")
    e = B.ratio(got[2], ref[2], what + " p' (E)")
    limit = B.MARGIN * max(1.0, rc)
    print(f"[cw] {what}: m' (R) {rm:.3g}, v' (R) {rv:.3g} against {B.RIGOROUS:g}; p' (E) {e:.3g} / {rc:.3g} / {limit:.3g}")
    return rm, rv, e, limit, rc


def passes(fig) -> bool:
    rm, rv, e, limit, _ = fig
    return rm <= B.RIGOROUS and rv <= B.RIGOROUS and e <= limit


def check(got, ref, cpu32, what: str):
    fig = judge(got, ref, cpu32, what)
    rm, rv, e, limit, _ = fig
    assert rm <= B.RIGOROUS, f"{what}: m' (R) ratio {rm:.3g} > {B.RIGOROUS:g}"
    assert rv <= B.RIGOROUS, f"{what}: v' (R) ratio {rv:.3g} > {B.RIGOROUS:g}"
    assert e <= limit, f"{what}: p' (E) ratio {e:.3g} > {limit:.3g}"
    return fig
