"""Test support for the graph baselines: a float64 restatement, on the CPU, of

  * torch_geometric's documented GINConv formula   out_i = nn((1 + eps) * x_i + sum_{j -> i} x_j),  edge_index[0] the source
    and [1] the target, with `nn` the network every GIN model of the reference builds: Linear, norm, act, Linear, norm, act
    (mp/graph_models.py:41-49, mp/ring_exp_models.py:86-94);
  * the `forward` of GIN0 / GIN / GIN0WithJK / GINWithJK, mp/graph_models.py:72-82 and :132-145: conv1, the convs,
    (JumpingKnowledge: 'cat' side by side, 'max' element-wise), the readout per graph, act(lin1), lin2 (eval: no dropout);
  * the `forward` of RingGIN, mp/ring_exp_models.py:117-127: init_linear, act(conv1), the convs, lin1 on the marked rows.

These functions are the yardstick of the graph baselines' kernel tests, evaluated from a model's state_dict in float64.  They
are tied to the reference by tests/golden/gin_family.npz (tools/gen_golden_options.py: the reference's own GIN0, GIN,
GIN0WithJK, GINWithJK and RingGIN behind a stand-in GINConv): tests/test_options_golden_host.py evaluates them from the stored
states and holds them to the reference's float64 outputs, layer by layer, at 1e-11.  Nothing here calls the code under test."""
import torch

ACT64 = {'id': lambda z: z, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
BN_EPS = 1e-5              # torch.nn.BatchNorm1d's default


def index_like_oriented(n: int, seed: int, long_row: int = 64, long_rows: bool = True) -> torch.Tensor:
    """The generator of tests/test_gpu_oriented.py::_index restated: a COO index [2, E] over n rows in shuffled entry order, most
    rows 0 .. 5 entries (a third of them empty) and -- as far as n has the rows -- one row of exactly `long_row` entries, one
    of long_row + 1, one of 300."""
    g = torch.Generator().manual_seed(seed)
    if n == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    deg = torch.randint(0, 6, (n,), generator=g)
    deg[torch.rand(n, generator=g) < 0.33] = 0
    if long_rows:
        for r, d in zip(torch.randperm(n, generator=g)[:3].tolist(), (long_row, long_row + 1, 300)):
            deg[r] = d
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(deg.sum()),), generator=g)
    p = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[p], dst[p]])


def aggregate64(x64, index, eps):
    """(1 + eps) * x_i + sum_{j -> i} x_j in float64; index None: no edges; eps a number or a float64 tensor of one element."""
    s = (1.0 + eps) * x64
    if index is not None and index.numel():
        s = s + torch.zeros_like(x64).index_add_(0, index[1], x64[index[0]])
    return s


def gin_formula64(x, index, eps, stages, act, act_post='id'):
    """The launch's formula in float64.  stages: two (W, b, scale, shift), any of b / scale / shift None."""
    h = aggregate64(x.double(), index, float(eps))
    for W, b, scale, shift in stages:
        h = h @ W.double().t()
        if b is not None:
            h = h + b.double()
        if scale is not None:
            h = h * scale.double()
        if shift is not None:
            h = h + shift.double()
        h = ACT64[act](h)
    return ACT64[act_post](h)


def _norm64(st, prefix, z):
    """An eval-mode BatchNorm1d from its state (absent: Identity); LayerNorm is told apart by having no running statistics."""
    if prefix + '.running_mean' in st:
        z = (z - st[prefix + '.running_mean']) / torch.sqrt(st[prefix + '.running_var'] + BN_EPS)
        return z * st[prefix + '.weight'] + st[prefix + '.bias']
    if prefix + '.weight' in st:
        return torch.nn.functional.layer_norm(z, (z.size(1),), st[prefix + '.weight'], st[prefix + '.bias'])
    return z


def conv64(st, prefix, x, index, act):
    """One GINConv from the model's float64 state: eps from `<prefix>.eps`, the network from `<prefix>.nn.{0,1,3,4}`."""
    h = aggregate64(x, index, st[prefix + '.eps'])
    for lin, norm in ((0, 1), (3, 4)):
        h = h @ st[f'{prefix}.nn.{lin}.weight'].t() + st[f'{prefix}.nn.{lin}.bias']
        h = ACT64[act](_norm64(st, f'{prefix}.nn.{norm}', h))
    return h


def state64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def _n_convs(st):
    return 1 + len({k.split('.')[1] for k in st if k.startswith('convs.')})


def gin_model64(st, x, index, batch, size, act='relu', readout='sum', jump=None, partial=False):
    """GIN0 / GIN (jump None) and GIN0WithJK / GINWithJK (jump 'cat' | 'max') in eval, from the float64 state."""
    x = x.double()
    xs = []
    for prefix in ['conv1'] + [f'convs.{i}' for i in range(_n_convs(st) - 1)]:
        x = conv64(st, prefix, x, index, act)
        xs.append(x)
    if jump == 'cat':
        x = torch.cat(xs, dim=-1)
    elif jump == 'max':
        x = torch.stack(xs, dim=-1).max(dim=-1)[0]
    cells = x
    pooled = torch.zeros(size, x.size(1), dtype=torch.float64).index_add_(0, batch, x)
    if readout == 'mean':
        pooled = pooled / torch.bincount(batch, minlength=size).clamp(min=1).double().unsqueeze(1)
    h = ACT64[act](pooled @ st['lin1.weight'].t() + st['lin1.bias'])
    out = h @ st['lin2.weight'].t() + st['lin2.bias']
    return (out, cells) if partial else out


def ring_gin64(st, x, index, mask, act='relu'):
    """RingGIN in eval, from the float64 state."""
    x = x.double() @ st['init_linear.weight'].t() + st['init_linear.bias']
    x = ACT64[act](conv64(st, 'conv1', x, index, act))
    for i in range(_n_convs(st) - 1):
        x = conv64(st, f'convs.{i}', x, index, act)
    return x[mask] @ st['lin1.weight'].t() + st['lin1.bias']


def randomise(model, seed: int):
    """Running statistics and affine terms of every BatchNorm1d away from (0, 1, 1, 0), and every trained eps away from 0, so
    that a comparison sees them; in place, returns the model."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.num_features, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=g))
            eps = getattr(m, 'eps', None)
            if isinstance(eps, torch.nn.Parameter):
                eps.fill_(0.1 + 0.5 * float(torch.rand(1, generator=g)))
    return model
