"""Operands, Tracked references and float32-torch restatements of the normalisation checks, shared by the CPU twins
(tests/test_bounds_host.py) and the kernels (tests/test_gpu_norm_componentwise.py).

BatchNorm: z [M, N] = graded_z (column spreads grade_cols, column means grade_ratio spreads), gamma in [0.5, 1.5), beta ~ randn,
dy ~ randn with columns graded by grade_cols, running statistics at the columns' own scale.  LayerNorm: rows graded by
grade_rows and offset by grade_ratio(M) spreads, gamma and dy columns graded by grade_cols."""
import torch
import torch.nn.functional as F

from tests import _bounds as B

EPS, MOM = 1e-5, 0.1
DISPUTED_CAP = 0.01            # the share of a matrix whose ReLU sign float32 and float64 may dispute: a condition, not a measurement


class BnCase:
    def __init__(self, M, N, seed=0, rows=False, relu=True, eps=EPS, z=None, module=None):
        """`z`: the pre-activation a launch stored (float32 [M, N]) in place of graded_z.  `module`: (gamma, beta, running_mean,
        running_var) of a BatchNorm of a model, as they stood BEFORE the launch, in place of the drawn ones."""
        g = torch.Generator().manual_seed(1000 * M + 10 * N + seed + 7 * rows)
        self.M, self.N, self.relu, self.eps = M, N, relu, eps
        self.gc = B.grade_cols(N)
        self.z = B.graded_z(g, M, N, rows) if z is None else z.detach().cpu().float()
        assert tuple(self.z.shape) == (M, N)
        self.gamma, self.beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
        self.rm0, self.rv0 = torch.randn(N, generator=g) * self.gc, (torch.rand(N, generator=g) + 0.5) * self.gc ** 2
        if module is not None:
            self.gamma, self.beta, self.rm0, self.rv0 = (t.detach().cpu().float().clone() for t in module)
        self.dy_plain = torch.randn(M, N, generator=g)
        self.what = f'M={M} N={N}{" rows" if rows else ""} relu={int(relu)}'
        # the gradient with the entries of a disputed ReLU sign set to zero: neither side's sums depend on the disputed mask
        y = self.fwd(B.FMA)['y']
        self.disputed = B.sign_disputed(y) if relu else torch.zeros(M, N, dtype=torch.bool)
        self.mask = (y.v > 0) if relu else torch.ones(M, N, dtype=torch.bool)
        self.dy_plain = self.dy_plain * (~self.disputed)
        self.dy = self.dy_plain * self.gc[None, :]
        self.dyh = self.dy * self.mask

    def share(self) -> float:
        s = float(self.disputed.double().mean())
        print(f'[cw] {self.what}: {int(self.disputed.sum())} of {self.disputed.numel()} entries have a disputed ReLU sign ({100 * s:.3g}%)')
        return s

    def stats(self, steps) -> B.BnStats:
        return B.bn_stats(self.z, self.eps, steps)

    def fwd(self, steps, unbiased_roundings=1) -> dict:
        st = self.stats(steps)
        scale, shift, y = B.bn_affine(self.z, st, self.gamma, self.beta)
        return dict(st=st, mean=st.mean, rstd=st.rstd, scale=scale, shift=shift, y=y, out=B.act(y, 'relu') if self.relu else y,
                    running_mean=B.bn_running(self.rm0, st.mean, MOM),
                    running_var=B.bn_running(self.rv0, B.bn_unbiased(st, unbiased_roundings), MOM))

    def bwd(self, steps, form='apply', dyh=None) -> dict:
        f = self.fwd(steps)
        dz, s1, s2 = B.bn_backward(self.z, self.dyh if dyh is None else dyh, f['st'], f['scale'], steps, form)
        return dict(dz=dz, s1=s1, s2=s2)

    def bwd_handed(self, steps, dy, form='stage') -> dict:
        """The backward behind a gradient this stage was HANDED (inside a plan: nothing can be zeroed where the ReLU sign is
        disputed): there dyh is dy or 0, so it travels as v = dy [y > 0] with an allowance of |dy| (c = |dy| / (2 unit)), which the
        sums and dz inherit; everywhere else it is an input."""
        dy = B._d(dy)
        dyh = B.Tracked(dy * self.mask, dy.abs() * self.disputed / (B.RIGOROUS * B.UNIT32))
        f = self.fwd(steps)
        dz, s1, s2 = B.bn_backward(self.z, dyh, f['st'], f['scale'], steps, form)
        return dict(dz=dz, s1=s1, s2=s2)

    def cpu32(self):
        """torch32() with the two constants F.batch_norm does not hand out: the float32 column mean and the rounded float64 rstd."""
        cpu = self.torch32()
        if cpu is not None:
            cpu.update(mean=self.z.mean(0), rstd=(1.0 / torch.sqrt(self.z.double().var(0, unbiased=False) + self.eps)).float())
        return cpu

    def torch32(self):
        """F.batch_norm(training=True) (+ ReLU) and its autograd in float32 on the CPU; None at M = 1, which torch refuses."""
        if self.M < 2:
            return None
        z = self.z.clone().requires_grad_(True)
        gam, bet = self.gamma.clone().requires_grad_(True), self.beta.clone().requires_grad_(True)
        rm, rv = self.rm0.clone(), self.rv0.clone()
        y = F.batch_norm(z, rm, rv, gam, bet, True, MOM, self.eps)
        out = torch.relu(y) if self.relu else y
        out.backward(self.dy)
        return dict(out=out.detach(), running_mean=rm, running_var=rv, dz=z.grad, s1=bet.grad, s2=gam.grad)

    def band_sums(self, z=None, band=32):
        """[2, bands, N] float64: what a statistics epilogue leaves of z."""
        z = (self.z if z is None else z).double()
        zp = torch.cat([z, z.new_zeros((-z.size(0)) % band, z.size(1))]).view(-1, band, z.size(1))
        return torch.stack([zp.sum(1), (zp * zp).sum(1)])


class LnCase:
    def __init__(self, M, N, seed=0, relu=True, affine=True):
        g = torch.Generator().manual_seed(1000 * M + 10 * N + seed)
        self.M, self.N, self.relu = M, N, relu
        self.gc = B.grade_cols(N)
        self.z = (torch.randn(M, N, generator=g) + B.grade_ratio(M)[:, None]) * B.grade_rows(M)[:, None]
        self.gamma = (torch.rand(N, generator=g) + 0.5) * self.gc if affine else None
        self.beta = torch.randn(N, generator=g) * self.gc if affine else None
        self.dy_plain = torch.randn(M, N, generator=g)
        self.what = f'layernorm M={M} N={N} relu={int(relu)}'
        y = self.fwd(B.FMA)['y']
        self.disputed = B.sign_disputed(y) if relu else torch.zeros(M, N, dtype=torch.bool)
        self.mask = (y.v > 0) if relu else torch.ones(M, N, dtype=torch.bool)
        self.dy_plain = self.dy_plain * (~self.disputed)
        self.dy = self.dy_plain * self.gc[None, :]
        self.dyh = self.dy * self.mask

    share = BnCase.share

    def fwd(self, steps) -> dict:
        return B.ln_forward(self.z, self.gamma, self.beta, EPS, steps, self.relu)

    def bwd(self, steps, dyh=None) -> dict:
        dz, dgamma, dbeta = B.ln_backward(self.z, self.dyh if dyh is None else dyh, self.gamma, self.fwd(steps), steps)
        return dict(dz=dz, dgamma=dgamma, dbeta=dbeta)

    def torch32(self):
        z = self.z.clone().requires_grad_(True)
        gam, bet = self.gamma.clone().requires_grad_(True), self.beta.clone().requires_grad_(True)
        y = F.layer_norm(z, (self.N,), gam, bet, EPS)
        out = torch.relu(y) if self.relu else y
        out.backward(self.dy)
        zd = self.z.double()
        return dict(out=out.detach(), dz=z.grad, dgamma=gam.grad, dbeta=bet.grad, mean=self.z.mean(1),
                    rstd=(1.0 / torch.sqrt(zd.var(1, unbiased=False) + EPS)).float())


def hold(got: dict, ref_of, cpu32, names, what, steps=B.FMA, assert_=True):
    """(R) and (E) of every named result; returns {name: (r, e, limit, rc)}.  `ref_of(steps)` a dict of Tracked, `cpu32` a dict of
    float32 results or None ((R) only)."""
    figs = {}
    for name in names:
        fn = B.check if assert_ else B.measure
        figs[name] = fn(got[name], lambda s: ref_of(s)[name], steps, None if cpu32 is None else cpu32[name], f'{what} {name}')
    return figs


def passes(fig) -> bool:
    r, e, limit, rc = fig
    return r <= B.RIGOROUS and (e is None or e <= limit)


def caught_by(fig) -> str:
    r, e, limit, rc = fig
    gates = [n for n, bad in (('(R)', r > B.RIGOROUS), ('(E)', e is not None and e > limit)) if bad]
    return ' and '.join(gates) if gates else 'NEITHER'
