"""Test support for the molecular graph baseline: a float64 restatement, on the CPU, of

  * torch_geometric 1.6.3's documented GINEConv formula   out_i = nn((1 + eps) * x_i + sum_{j -> i} relu(x_j + e_ji)),
    edge_index[0] the source and [1] the target, with `nn` the network EmbedGIN builds: Linear, BatchNorm, act, Linear,
    BatchNorm, act (mp/molec_models.py:538-550);
  * the `forward` of EmbedGIN in eval, mp/molec_models.py:561-603: the embedding front over vertices and edges
    (mp/layers.py:490-570: the edges' rows are their embedded features, or the reduction of their two vertices' embeddings
    where they have none), the GINEConv layers over the vertex graph with the edge cochain's rows as edge features (the row
    `shared_coboundaries[p]` for entry p of `upper_index`), the readout over the vertices, act(lin1), lin2.

These functions are the yardstick of the GINE kernel's tests, evaluated from a model's state_dict in float64.  They are tied to
the reference by tests/golden/gin_family.npz (tools/gen_golden_options.py: the reference's own EmbedGIN behind a stand-in
GINEConv, five configurations): tests/test_options_golden_host.py evaluates them from the stored states and holds them to the
reference's float64 outputs at 1e-11.  Nothing here calls the code under test."""
import torch

from tests._gin import ACT64, _norm64

REDUCE64 = {'sum': 'sum', 'add': 'sum', 'mean': 'mean', 'max': 'amax', 'min': 'amin'}


def messages64(x64, index, e64, eidx_mode):
    """sum_{j -> i} relu(x_j + e_ji) in float64.  index [2, E] (None: no edges); eidx_mode: 'perm' -- e64 holds one row per
    entry of `index` -- or an int64 [E] tensor -- entry p reads the row eidx_mode[p] of e64 (the shared-cell index)."""
    s = torch.zeros_like(x64)
    if index is not None and index.numel():
        rows = e64 if isinstance(eidx_mode, str) else e64[eidx_mode]
        assert isinstance(eidx_mode, torch.Tensor) or eidx_mode == 'perm'
        s.index_add_(0, index[1], torch.relu(x64[index[0]] + rows))
    return s


def gine_formula64(x, index, e, eidx_mode, eps, stages, act, act_post='id'):
    """The launch's formula in float64.  stages: two (W, b, scale, shift), any of b / scale / shift None."""
    x64 = x.double()
    h = messages64(x64, index, None if e is None else e.double(), eidx_mode) + (1.0 + float(eps)) * x64
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


def conv64(st, prefix, x, index, e, eidx_mode, act):
    """One GINEConv from the model's float64 state: eps from `<prefix>.eps`, the network from `<prefix>.nn.{0,1,3,4}`."""
    h = messages64(x, index, e, eidx_mode) + (1.0 + st[prefix + '.eps']) * x
    for lin, norm in ((0, 1), (3, 4)):
        h = h @ st[f'{prefix}.nn.{lin}.weight'].t() + st[f'{prefix}.nn.{lin}.bias']
        h = ACT64[act](_norm64(st, f'{prefix}.nn.{norm}', h))
    return h


def embed_gin64(st, v_x, e_x, boundary_index, n_edges, upper_index, shared, batch, size, act='relu', readout='sum',
                init_reduce='sum', partial=False):
    """EmbedGIN in eval, from the float64 state and the plain tensors of a (batched) complex:
    v_x [n0, 1] the atom types; e_x [n1, 1] the bond types or None; boundary_index [2, B] of the edges (row 0 a vertex,
    row 1 its edge) or None without edges; n_edges = n1; upper_index [2, E] / shared [E] of the vertices (None: no edges);
    batch [n0] and the number of complexes."""
    x = st['v_embed_init.weight'][v_x.view(-1).long()]
    e = None
    if upper_index is not None:
        if e_x is not None:
            e = st['e_embed_init.weight'][e_x.view(-1).long()]
        else:
            rows, cells = x[boundary_index[0]], boundary_index[1]
            e = torch.zeros(n_edges, x.size(1), dtype=torch.float64).scatter_reduce(
                0, cells.unsqueeze(1).expand_as(rows), rows, REDUCE64[init_reduce], include_self=False)
    n_layers = len({k.split('.')[1] for k in st if k.startswith('convs.')})
    for i in range(n_layers):
        x = conv64(st, f'convs.{i}', x, upper_index, e, shared, act)
    cells = x
    pooled = torch.zeros(size, x.size(1), dtype=torch.float64).index_add_(0, batch, x)
    if readout == 'mean':
        pooled = pooled / torch.bincount(batch, minlength=size).clamp(min=1).double().unsqueeze(1)
    h = ACT64[act](pooled @ st['lin1.weight'].t() + st['lin1.bias'])
    out = h @ st['lin2.weight'].t() + st['lin2.bias']
    return (out, cells) if partial else out


def embed_gin64_of(st, batch, **kw):
    """embed_gin64 on a CPU ComplexBatch / Complex of this project's containers (read for their plain tensors alone)."""
    v = batch.cochains[0]
    e = batch.cochains.get(1) if v.upper_index is not None else None
    vb = getattr(v, 'batch', None)
    if vb is None:
        vb = torch.zeros(v.x.size(0), dtype=torch.long)
    size = getattr(batch, 'num_complexes', None) or int(vb.max()) + 1
    return embed_gin64(st, v.x, None if e is None else e.x, None if e is None else e.boundary_index,
                       0 if e is None else e.num_cells, v.upper_index, v.shared_coboundaries if e is not None else None,
                       vb, size, **kw)
