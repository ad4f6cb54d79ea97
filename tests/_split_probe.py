"""Inputs with an exact answer for the bf16 three-way split (csrc/cwn_split.h), and a CPU model of the split.

A product x*w on the split path is six bf16 piece products (wh*xh, wh*xm, wm*xh, wm*xm, wh*xl, wl*xh) summed in fp32.  The
probes here are integer matrices for which
  * every KEPT term of a class is exercised (non-zero on most outputs),
  * every DROPPED term (wm*xl, wl*xm, wl*xl) is exactly zero because one factor is zero, and
  * every partial sum, in any order, is an integer below 2^24 and therefore exact in fp32,
so a kernel that implements the split must return the int64 product under torch.equal -- no tolerance.  A kernel that lost a
term, or laid one plane of one operand out under another contraction index than the others, returns other integers.
`emulate` is that statement as a CPU model (float64 over the CPU pieces), with the two faults as switches;
tests/test_split_probe_host.py uses it to prove, without a GPU, that the inputs see the faults they are for.

Value pools (integers; `split` decides membership, not the bit count):
  one    one piece:    +-1, +-2, +-3                                   (mid = lo = 0)
  two    two pieces:   9- and 10-bit integers with mid != 0, lo == 0   (`cap`: the layer tests, which sum further, stay below 768)
  three  three pieces: 18-bit integers with mid != 0, lo != 0
(An integer of up to 17 bits never has a third piece: round-to-nearest leaves a residual of at most half an ulp of `hi`,
|r| <= 2^8, and every such integer is a bf16 number.  18 bits is the narrowest pool in which `lo` exists.)

Operand classes, X [M, K] times W [N, K] over K:
  A   X from three, W from one    terms wh*xh, wh*xm, wh*xl
  B   X from one,   W from three  terms wh*xh, wm*xh, wl*xh
  C   X and W from two            terms wh*xh, wh*xm, wm*xh, wm*xm
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

TERMS = ('wh*xh', 'wh*xm', 'wm*xh', 'wm*xm', 'wh*xl', 'wl*xh')          # the six the kernels keep (w plane, x plane)
DROPPED = ('wm*xl', 'wl*xm', 'wl*xl')
CLASS_POOLS = {'A': ('three', 'one'), 'B': ('one', 'three'), 'C': ('two', 'two')}          # (pool of X, pool of W)
CLASS_TERMS = {'A': ('wh*xh', 'wh*xm', 'wh*xl'), 'B': ('wh*xh', 'wm*xh', 'wl*xh'), 'C': ('wh*xh', 'wh*xm', 'wm*xh', 'wm*xm')}
# the planes that are non-zero in a class: (operand, plane)
CLASS_PLANES = {'A': (('x', 'h'), ('x', 'm'), ('x', 'l'), ('w', 'h')),
                'B': (('x', 'h'), ('w', 'h'), ('w', 'm'), ('w', 'l')),
                'C': (('x', 'h'), ('x', 'm'), ('w', 'h'), ('w', 'm'))}
EXACT_LIMIT = 1 << 24                  # integers below it are fp32 numbers, and so are all their sums below it
LAYER_CAP_C = 768                      # class C in the blocked-layer tests: |value| below it (ten messages of two products each)
MAX_NNZ = 8                            # non-zero entries along the contraction index, per output element


def split(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(hi, mid, lo) of fp32 `x`, each an fp32 tensor that holds a bf16 number; round to nearest even at every step."""
    x = x.detach().cpu().float()
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = x - hi - mid
    assert torch.equal(hi + mid + lo, x), 'the three pieces do not add up to x'
    assert torch.equal(lo.bfloat16().float(), lo), 'lo is not a bf16 number'
    return hi, mid, lo


def _filtered(cands: torch.Tensor, want_mid: bool, want_lo: bool) -> torch.Tensor:
    _, mid, lo = split(cands.float())
    keep = ((mid != 0) == want_mid) & ((lo != 0) == want_lo)
    vals = cands[keep]
    return torch.cat([vals, -vals])


def pool(name: str) -> torch.Tensor:
    """All members of a value pool (int64, both signs)."""
    if name == 'one':
        return _filtered(torch.arange(1, 4), False, False)
    if name == 'two':
        return _filtered(torch.arange(1 << 8, 1 << 10), True, False)
    if name == 'three':
        return _filtered(torch.arange(1 << 17, 1 << 18), True, True)
    raise KeyError(name)


_POOLS = {}


def draw(name: str, shape, gen: torch.Generator, p_neg: float = 0.5, cap: int = 0) -> torch.Tensor:
    """int64 draws from a pool; `p_neg` is the share of negative values, `cap` (if set) an exclusive bound on |value|."""
    if name not in _POOLS:
        _POOLS[name] = pool(name)
    vals = _POOLS[name]
    pos = vals[:vals.numel() // 2]                 # (the first half is positive, the second its mirror image)
    if cap:
        pos = pos[pos < cap]
    mag = pos[torch.randint(0, pos.numel(), tuple(shape), generator=gen)]
    neg = torch.rand(tuple(shape), generator=gen) < p_neg
    return torch.where(neg, -mag, mag)


def sparse_rows(name: str, M: int, K: int, nnz: int, gen: torch.Generator, p_neg: float = 0.5, cap: int = 0) -> torch.Tensor:
    """[M, K] int64 with `nnz` non-zero entries per row: one at column (37 r + 5) % K -- 37 is odd, so K consecutive rows
    cover every column when K is a power of two -- and the others drawn."""
    assert 1 <= nnz <= min(K, MAX_NNZ)
    out = torch.zeros(M, K, dtype=torch.int64)
    r = torch.arange(M)
    forced = (37 * r + 5) % K
    # nnz - 1 further distinct columns per row, none of them the forced one: offsets 1 .. K-1 from it
    offs = torch.rand(M, K - 1, generator=gen).argsort(1)[:, :nnz - 1] + 1
    cols = torch.cat([forced[:, None], (forced[:, None] + offs) % K], 1)
    out.scatter_(1, cols, draw(name, (M, nnz), gen, p_neg, cap))
    return out


def pieces_abs(x: torch.Tensor) -> torch.Tensor:
    """|hi| + |mid| + |lo| (float64): what bounds any partial sum of piece products."""
    h, m, l = split(x.float())
    return h.double().abs() + m.double().abs() + l.double().abs()


def assert_exact(X: torch.Tensor, W: torch.Tensor, what: str = '') -> float:
    """The condition under which torch.equal is a legitimate assertion for X [M, K] times W [N, K] over K (unscaled integer
    operands): every dropped term is zero, and the absolute piece products of every output element sum to < 2^24, so any
    subset of them summed in any order in fp32 is exact.  Returns the largest such sum."""
    assert X.dtype == torch.int64 and W.dtype == torch.int64
    assert float(X.abs().max()) < EXACT_LIMIT and float(W.abs().max()) < EXACT_LIMIT
    xh, xm, xl = split(X.float())
    wh, wm, wl = split(W.float())
    for a, b, name in ((wm, xl, 'wm*xl'), (wl, xm, 'wl*xm'), (wl, xl, 'wl*xl')):
        assert float((b.double().abs() @ a.double().abs().t()).max()) == 0.0, f'{what}: the dropped term {name} is not zero'
    assert int((X != 0).sum(1).max()) <= MAX_NNZ or int((W != 0).sum(1).max()) <= MAX_NNZ, what
    top = float((pieces_abs(X) @ pieces_abs(W).t()).max())
    assert top < EXACT_LIMIT, f'{what}: absolute terms sum to {top:.0f} >= 2^24'
    return top


@dataclass
class Probe:
    cls: str
    X: torch.Tensor            # [M, K] fp32 (scaled when the case is)
    W: torch.Tensor            # [N, K] fp32
    ref: torch.Tensor          # [M, N] float64: the exact X W^T
    Xi: torch.Tensor           # the unscaled integers
    Wi: torch.Tensor
    top: float                 # the largest sum of absolute piece products of an output element (< 2^24)
    ex: Optional[torch.Tensor] = None      # exponents of the power-of-two scales: rows of X, rows of W (= output columns)
    ew: Optional[torch.Tensor] = None

    def scaled_like_ref(self, t: torch.Tensor) -> torch.Tensor:
        """An integer [M, N] result in the scale of `ref` (float64)."""
        t = t.double()
        return t if self.ex is None else torch.ldexp(t, self.ex[:, None] + self.ew[None, :])


def scales(n: int, gen: torch.Generator) -> torch.Tensor:
    """n exponents in [-30, 30].  Pieces stay normal: the smallest, |x| * 2^-18 * 2^-30, is far above 2^-126."""
    return torch.randint(-30, 31, (n,), generator=gen)


def make_case(cls: str, M: int, N: int, K: int, nnz: int = MAX_NNZ, seed: int = 0, scaled: bool = False, w_nnz: int = 0,
              p_neg: float = 0.5, cap: int = 0) -> Probe:
    """One probe of class `cls`: X [M, K] with `nnz` non-zeros per row (covering every k and every row position), W [N, K]
    dense (or `w_nnz` non-zeros per row), the exact product, checked by assert_exact."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K + ord(cls))
    px, pw = CLASS_POOLS[cls]
    Xi = sparse_rows(px, M, K, nnz, gen, p_neg, cap)
    Wi = sparse_rows(pw, N, K, w_nnz, gen, p_neg, cap) if w_nnz else draw(pw, (N, K), gen, p_neg, cap)
    top = assert_exact(Xi, Wi, f'class {cls} {M}x{N}x{K}')
    assert M < K or bool((Xi != 0).any(0).all()), 'a contraction index is never exercised'
    ref = (Xi @ Wi.t()).double()
    X, W, ex, ew = Xi.float(), Wi.float(), None, None
    if scaled:
        ex, ew = scales(M, gen), scales(N, gen)
        X = torch.ldexp(X, ex[:, None])
        W = torch.ldexp(W, ew[:, None])
        ref = torch.ldexp(ref, (ex[:, None] + ew[None, :]))
        assert torch.equal(ref.float().double(), ref)
    return Probe(cls, X, W, ref, Xi, Wi, top, ex, ew)


@dataclass
class TnProbe:
    cls: str
    dZ: torch.Tensor           # [M, N] fp32, one non-zero per live row
    X: torch.Tensor            # [M, K] fp32, dense
    dZi: torch.Tensor          # the unscaled integers
    Xi: torch.Tensor
    en: Optional[torch.Tensor] = None      # exponents of the power-of-two scales: columns of dZ, columns of X
    ek: Optional[torch.Tensor] = None

    def ref(self, relu_cols: int = 0) -> torch.Tensor:
        """dZ^T X in float64 ([N, K]), with ReLU on the first `relu_cols` columns of X."""
        Xi = self.Xi.clone()
        Xi[:, :relu_cols].clamp_(min=0)
        out = (self.dZi.t() @ Xi).double()
        return out if self.en is None else torch.ldexp(out, self.en[:, None] + self.ek[None, :])

    def ref_db(self) -> torch.Tensor:
        out = self.dZi.sum(0).double()
        return out if self.en is None else torch.ldexp(out, self.en)


def make_tn_case(cls: str, M: int, N: int, K: int, live: Optional[torch.Tensor] = None, seed: int = 0,
                 scaled: bool = False) -> TnProbe:
    """A weight-gradient probe dW = dZ^T X: the contraction runs over the M rows.  X [M, K] is dense from the class's X pool;
    dZ [M, N] (from the W pool) has one non-zero in each of the `live` rows (default: all M, M = 8 N), placed so that every
    column receives MAX_NNZ rows, N rows apart -- different 32-row chunks of a band -- at a row position that moves by 5 from
    one to the next."""
    gen = torch.Generator().manual_seed(2000 * seed + 7 * M + 3 * N + K + ord(cls))
    px, pw = CLASS_POOLS[cls]
    live = torch.arange(M) if live is None else live
    assert live.numel() == MAX_NNZ * N and int(live.max()) < M and live.unique().numel() == live.numel()
    Xi = draw(px, (M, K), gen)
    j = torch.arange(live.numel())
    dZi = torch.zeros(M, N, dtype=torch.int64)
    dZi[live, (j + 5 * (j // N)) % N] = draw(pw, (live.numel(),), gen)
    assert int((dZi != 0).sum(0).min()) == MAX_NNZ == int((dZi != 0).sum(0).max())
    assert_exact(dZi.t().contiguous(), Xi.t().contiguous(), f'class {cls} weight gradient {M}x{N}x{K}')
    assert float(pieces_abs(dZi).sum(0).max()) < EXACT_LIMIT            # (the bias gradient: column sums of dZ)
    p = TnProbe(cls, dZi.float(), Xi.float(), dZi, Xi)
    if scaled:
        p.en, p.ek = scales(N, gen), scales(K, gen)
        p.dZ, p.X = torch.ldexp(p.dZ, p.en[None, :]), torch.ldexp(p.X, p.ek[None, :])
    return p


def emulate(X: torch.Tensor, W: torch.Tensor, drop: Optional[str] = None, roll: Optional[Tuple[str, str]] = None) -> torch.Tensor:
    """The six-term sum of X [M, K] times W [N, K] in float64 from the CPU pieces.  `drop` leaves one of TERMS out;
    `roll=(operand, plane)` moves one plane ('h', 'm', 'l') of one operand ('x', 'w') by one position along the contraction
    index: the plane read under another bijection than its siblings."""
    assert drop is None or drop in TERMS
    planes = {'x': dict(zip('hml', (p.double() for p in split(X)))), 'w': dict(zip('hml', (p.double() for p in split(W))))}
    if roll is not None:
        op, pl = roll
        planes[op][pl] = torch.roll(planes[op][pl], 1, dims=1)
    out = torch.zeros(X.size(0), W.size(0), dtype=torch.float64)
    for term in TERMS:
        if term != drop:
            out += planes['x'][term[4]] @ planes['w'][term[1]].t()
    return out


def changed_share(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Share of the non-zero outputs of `ref` that `got` gets wrong."""
    nz = ref != 0
    return float(((got != ref) & nz).sum()) / max(int(nz.sum()), 1)


# The products the GPU tests (tests/test_gpu_split_terms.py) run, by site, as make_case arguments (M, N, K, non-zeros per
# row of X); the host test checks the fault matrix at each.  The weight gradient (make_tn_case) is listed there.
SHAPES = {
    'gemm': (256, 128, 128, 8),
    'gemm-multi': (512, 128, 128, 8),
    'stage64-single': (2048 // 64 + 1, 64, 64, 8),
    'stage64-cat': (2048 // 64 + 1, 64, 128, 8),
    'stage64-ex3': (2048 // 64 + 1, 64, 192, 8),
    'stage64-ex4': (256 * 64 + 37, 64, 256, 8),
    'stage128-single': (2048 // 128 + 1, 128, 128, 8),
    'stage128-cat': (256 * 32 + 37, 128, 256, 8),
    'stage128-ex3': (2048 // 128 + 1, 128, 384, 8),
    'stage128-ex4': (2048 // 128 + 1, 128, 512, 8),
    'stage64-bwd-wide': (2048 // 64 + 1, 128, 64, 8),
    'stage128-bwd': (2048 // 128 + 1, 128, 128, 8),
    'mlp64': (65, 64, 64, 8),
    'mlp64-combine': (131, 64, 128, 8),
    'mlp128': (33, 128, 128, 8),
    'mlp3-128-combine': (67, 128, 384, 8),
    'layer64': (300, 64, 128, 2),           # [x_j | x_shared] W^T of the blocked layer: at most 2 features per row
    'layer128': (300, 128, 256, 2),
}
TN_SHAPES = {'gemm_tn': (1024, 128, 128), 'gemm_tn-cat': (1024, 128, 256)}
