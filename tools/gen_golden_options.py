"""tests/golden/cell_options.npz and tests/golden/gin_family.npz: the reference's own models run at the options no other fixture
covers -- non-ReLU nonlinearities, graph_norm 'ln' and 'id', jump_mode 'max', and the graph baselines GIN0 / GIN / GIN0WithJK /
GINWithJK / RingGIN / EmbedGIN.

    python tools/gen_golden_options.py            # write the two fixtures
    python tools/gen_golden_options.py --check    # regenerate in memory and compare with the committed files, byte for byte

CPU only.  The reference is imported behind the stand-ins of oracle/refshim exactly as oracle/gen_golden.py imports it (that
module is read, not changed: its path setup, `get`, `np_`, `dump_complex` and `save` are used from here).  The graph baselines
run behind the stand-in GINConv / GINEConv of oracle/refshim/torch_geometric/nn, written from torch_geometric 1.6.3's documented
formulas; `check_gin_known_answers` pins both against a hand-computed answer before anything is written, as
gen_golden.check_reference_known_answers pins the scatter stand-ins.  The forward hooks that record the per-layer outputs of the
graph models (and of EmbedSparseCINNoRings, whose forward has no include_partial) are this file's own code.

What is written is data: inputs, batched index tensors, per case a JSON string of the constructor's settings ('<case>/cfg'), the
float32 state_dict ('<case>/state/...'), and the outputs: '<case>/out64' and '<case>/p64/<name>' from `model.double()` on float64
features, '<case>/out32' from the float32 model (its partials are checked against the condition below, not stored).  Every case
has dropout_rate 0, randomised BatchNorm running statistics (as oracle/gen_golden.py), norm affine terms away from (1, 0) and
every trained eps away from 0.  The
reference allocates its pooled matrix in the default dtype, so the float64 run is under torch.set_default_dtype(float64), as
exp/run_sr_exp.py runs.

cell_options.npz -- eval mode, 2 layers, the MOL_LIST batch with integer atom / bond types unless said otherwise:
   1 elu_bn_cob     EmbedSparseCIN 16 elu bn, use_coboundaries
   2 tanh_ln_cat    EmbedSparseCIN 16 tanh ln, readout mean, final_readout mean, jump_mode cat, train_eps
   3 sigmoid_id     EmbedSparseCIN 16 sigmoid id, no coboundaries
   4 id_bn          EmbedSparseCIN 16 id bn
   5 sr_elu_bn_64   SparseCIN 64 elu bn, use_coboundaries, float features, the SR(16,6,2,2) lifts of tools/gen_golden_agnostic.py
                    (rings up to 6; the lift's constant features plus seeded noise, so that rows differ)
   6 cinpp_elu      EmbedCINpp 16 elu bn
   7 ogb_tanh       OGBEmbedSparseCIN 16 tanh bn (OGB atom / bond feature columns)
   8 norings_elu    EmbedSparseCINNoRings 16 elu bn
   9 relu_ln_48     EmbedSparseCIN 48 relu ln
  10 relu_ln_10     EmbedSparseCIN 10 relu ln
  11 jk_max         EmbedSparseCIN 16 relu bn, jump_mode 'max': the reference's EmbedSparseCIN (and SparseCIN) accept it behind the
                    stand-in JumpingKnowledge
gin_family.npz -- eval mode; the graph of tests/_gin.index_like_oriented(130, seed) (rows of 0, 64, 65 and 300 entries) cut into
4 graphs by a sorted batch vector plus one graph of 3 vertices without edges, a `mask` of one vertex per graph for RingGIN;
EmbedGIN on the MOL_LIST batch (and on a batch of fullstop / colon complexes: the reference's `edge_index is None` branch).
Training part, float64 only ('train/<case>/...'): case 1 and GIN (elu) in train() mode -- the output, the cotangent c and the
gradient of every parameter for loss = (out * c).sum(); 'train/<case>/grad32_err/<name>' is max |g32 - g64| of the REFERENCE's
own float32 autograd, the figure a float32 implementation's bound may be derived from.

Condition on the inputs, asserted before anything is written: for every stored tensor the reference's own float32 run stays
within half the project's gate of its float64 run, |t32 - t64| <= 0.5e-5 * max(1, |t64|_inf).
"""
import copy
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402  (puts oracle/refshim and the reference on sys.path)
from data.complex import Cochain as RefCochain, Complex as RefComplex, ComplexBatch as RefBatch  # noqa: E402
import mp.models as RM  # noqa: E402
import mp.molec_models as RMM  # noqa: E402
import mp.graph_models as RGM  # noqa: E402
import mp.ring_exp_models as RRM  # noqa: E402
from torch_geometric.nn import GINConv, GINEConv  # noqa: E402  (the stand-ins)
from ogb.graphproppred.mol_encoder import ATOM_DIMS, BOND_DIMS  # noqa: E402

from cwn_amd import synthetic  # noqa: E402
from tests._gin import index_like_oriented  # noqa: E402

CELL, GIN = 'cell_options.npz', 'gin_family.npz'
HALF_GATE = 0.5e-5
INDEX_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')
EMBED = dict(dropout_rate=0.0, max_dim=2, jump_mode=None, readout='sum', train_eps=False, final_hidden_multiplier=2,
             final_readout='sum', apply_dropout_before='lin2', init_reduce='sum', embed_edge=True, use_coboundaries=True)

# name -> (class, positional arguments, keyword arguments, input batch)
CELL_CASES = {
    'elu_bn_cob': ('EmbedSparseCIN', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='elu', graph_norm='bn'), 'mol'),
    'tanh_ln_cat': ('EmbedSparseCIN', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='tanh', graph_norm='ln', readout='mean',
                                                             final_readout='mean', jump_mode='cat', train_eps=True), 'mol'),
    'sigmoid_id': ('EmbedSparseCIN', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='sigmoid', graph_norm='id',
                                                            use_coboundaries=False), 'mol'),
    'id_bn': ('EmbedSparseCIN', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='id', graph_norm='bn'), 'mol'),
    'sr_elu_bn_64': ('SparseCIN', [1, 4, 2, 64], dict(dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='elu', readout='sum',
                                                     train_eps=False, final_hidden_multiplier=2, use_coboundaries=True,
                                                     final_readout='sum', graph_norm='bn'), 'sr'),
    'cinpp_elu': ('EmbedCINpp', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='elu', graph_norm='bn', train_eps=True), 'mol'),
    'ogb_tanh': ('OGBEmbedSparseCIN', [1, 2, 16], dict(dropout_rate=0.0, indropout_rate=0.0, max_dim=2, jump_mode=None,
                                                       nonlinearity='tanh', readout='mean', final_readout='sum', init_reduce='sum',
                                                       embed_edge=True, use_coboundaries=True, graph_norm='bn'), 'ogb'),
    'norings_elu': ('EmbedSparseCINNoRings', [28, 4, 1, 2, 16], dict(dropout_rate=0.0, nonlinearity='elu', readout='sum',
                                                                    train_eps=False, final_hidden_multiplier=2, final_readout='sum',
                                                                    init_reduce='sum', embed_edge=True, use_coboundaries=True,
                                                                    graph_norm='bn'), 'mol'),
    'relu_ln_48': ('EmbedSparseCIN', [28, 4, 1, 2, 48], dict(EMBED, nonlinearity='relu', graph_norm='ln'), 'mol'),
    'relu_ln_10': ('EmbedSparseCIN', [28, 4, 1, 2, 10], dict(EMBED, nonlinearity='relu', graph_norm='ln'), 'mol'),
    'jk_max': ('EmbedSparseCIN', [28, 4, 1, 2, 16], dict(EMBED, nonlinearity='relu', graph_norm='bn', jump_mode='max'), 'mol'),
}
CLASSES = 4
GIN_CASES = {   # (class, [num_features, num_layers, hidden, num_classes], keyword arguments)
    'gin0_relu': ('GIN0', [5, 3, 16, CLASSES], dict(readout='sum', dropout_rate=0.0, nonlinearity='relu')),
    'gin_elu': ('GIN', [12, 3, 48, CLASSES], dict(readout='mean', dropout_rate=0.0, nonlinearity='elu')),
    'gin0jk_cat_tanh': ('GIN0WithJK', [12, 3, 48, CLASSES], dict(mode='cat', readout='sum', dropout_rate=0.0, nonlinearity='tanh')),
    'ginjk_max_sigmoid': ('GINWithJK', [5, 3, 16, CLASSES], dict(mode='max', readout='sum', dropout_rate=0.0, nonlinearity='sigmoid')),
    'gin0_id_64': ('GIN0', [64, 2, 64, CLASSES], dict(readout='sum', dropout_rate=0.0, nonlinearity='id')),
    'ring_bn': ('RingGIN', [5, 3, 16, CLASSES], dict(nonlinearity='relu', graph_norm='bn')),
    'ring_ln': ('RingGIN', [12, 3, 48, CLASSES], dict(nonlinearity='relu', graph_norm='ln')),
}
EGIN = dict(dropout_rate=0.0, nonlinearity='relu', readout='sum', train_eps=False, apply_dropout_before='lin2', init_reduce='sum',
            embed_edge=True, embed_dim=None)
EGIN_CASES = {  # (positional arguments, keyword arguments, input batch)
    'egin_edge': ([28, 4, 1, 2, 16], dict(EGIN), 'mol'),
    'egin_noedge': ([28, 4, 1, 2, 16], dict(EGIN, embed_edge=False, init_reduce='mean', nonlinearity='elu', readout='mean',
                                           train_eps=True), 'mol_noedge'),
    'egin_dim12': ([28, 4, 1, 1, 16], dict(EGIN, embed_dim=12), 'mol'),
    'egin_nodes_only': ([28, 4, 1, 2, 16], dict(EGIN), 'nodes_only'),
    'egin_lin1': ([28, 4, 1, 2, 16], dict(EGIN, apply_dropout_before='lin1'), 'mol'),
}
NODES_ONLY = ['fullstop', 'colon', 'colon', 'fullstop', 'colon']
TRAIN_CASES = ('elu_bn_cob', 'gin_elu')


# ------------------------------------------------------------------------------------------------
# the stand-ins against a hand-computed answer
# ------------------------------------------------------------------------------------------------
def check_gin_known_answers():
    """A path 0 - 1 - 2 (both directions) and one extra directed edge 0 -> 2; x = [[1, 2], [3, 5], [7, 11]]; nn = Identity.
    Sources per target: 0 <- {1}; 1 <- {0, 2}; 2 <- {1, 0}.
    GIN, eps 0.5:  row i = 1.5 x_i + sum of its sources' rows.
    GINE, eps 0, edge features e_p = [p - 2, 2 - p] for entry p = 0..4 of (src, dst) = (0,1) (1,0) (1,2) (2,1) (0,2):
    row i = x_i + sum relu(x_src + e_p)."""
    index = torch.tensor([[0, 1, 1, 2, 0], [1, 0, 2, 1, 2]])
    x = torch.tensor([[1., 2.], [3., 5.], [7., 11.]])
    gin = GINConv(torch.nn.Identity(), eps=0.5, train_eps=True)
    assert isinstance(gin.eps, torch.nn.Parameter) and 'eps' in gin.state_dict()
    # 0: 1.5 * [1, 2] + [3, 5];  1: 1.5 * [3, 5] + [1, 2] + [7, 11];  2: 1.5 * [7, 11] + [3, 5] + [1, 2]
    assert gin(x, index).tolist() == [[4.5, 8.0], [12.5, 20.5], [14.5, 23.5]]
    gin0 = GINConv(torch.nn.Identity())
    assert not isinstance(gin0.eps, torch.nn.Parameter) and gin0.state_dict()['eps'].tolist() == [0.0]
    assert gin0(x, index).tolist() == [[4., 7.], [11., 18.], [11., 18.]]
    e = torch.tensor([[-2., 2.], [-1., 1.], [0., 0.], [1., -1.], [2., -2.]])
    gine = GINEConv(torch.nn.Identity())
    # messages: p0 (0 -> 1) relu([1, 2] + [-2, 2]) = [0, 4];  p1 (1 -> 0) relu([3, 5] + [-1, 1]) = [2, 6];
    #           p2 (1 -> 2) [3, 5];  p3 (2 -> 1) relu([7, 11] + [1, -1]) = [8, 10];  p4 (0 -> 2) relu([1, 2] + [2, -2]) = [3, 0]
    # 0: [1, 2] + [2, 6];  1: [3, 5] + [0, 4] + [8, 10];  2: [7, 11] + [3, 5] + [3, 0]
    assert gine(x, index, e).tolist() == [[3., 8.], [11., 19.], [13., 16.]]
    gine.eps.data.fill_(0.25)
    gine.reset_parameters()
    assert gine.eps.tolist() == [0.0]
    empty = torch.LongTensor([[], []])
    assert gine(x, empty, torch.zeros(1, 2)).tolist() == x.tolist() and gin0(x, empty).tolist() == x.tolist()
    print('GINConv / GINEConv stand-ins reproduce the hand-computed answers')


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def mol_complexes(kind, gen):
    """MOL_LIST with integer atom / bond types ('mol': one column, as ZINC; 'ogb': the OGB feature columns; 'mol_noedge': the
    edges without features, what EmbedGIN(embed_edge=False) requires); 'nodes_only': fullstop / colon complexes."""
    cxs = [G.get(n) for n in (NODES_ONLY if kind == 'nodes_only' else G.MOL_LIST)]
    for cx in cxs:
        n0 = cx.cochains[0].num_cells
        if kind == 'ogb':
            cx.cochains[0]._Cochain__x = torch.stack([torch.randint(0, d, (n0,), generator=gen) for d in ATOM_DIMS], 1)
        else:
            cx.cochains[0]._Cochain__x = torch.randint(0, 28, (n0, 1), generator=gen).float()
        if cx.dimension >= 1:
            n1 = cx.cochains[1].num_cells
            if kind == 'ogb':
                cx.cochains[1]._Cochain__x = torch.stack([torch.randint(0, d, (n1,), generator=gen) for d in BOND_DIMS], 1)
            elif kind == 'mol_noedge':
                cx.cochains[1]._Cochain__x = None
            else:
                cx.cochains[1]._Cochain__x = torch.randint(0, 4, (n1, 1), generator=gen).float()
        if cx.dimension >= 2:
            cx.cochains[2]._Cochain__x = None
    return cxs


def sr_complexes(gen):
    """The rook's graph, a relabelled copy, the Shrikhande graph, a relabelled copy (tools/gen_golden_agnostic.py:sr_complexes,
    rings up to 6) in the reference's containers; features: the lift's plus seeded noise, float32-representable."""
    rng = np.random.default_rng(43)
    out = []
    for g in (synthetic.rook_4x4(), synthetic.shrikhande()):
        for cx in (synthetic.sr_lift(*g, max_k=6), synthetic.sr_lift(*synthetic.relabel(*g, rng.permutation(16)), max_k=6)):
            cochains = []
            for d in range(cx.dimension + 1):
                c = cx.cochains[d]
                kw = {k: c[k].clone() for k in INDEX_KEYS if c[k] is not None}
                kw['num_cells_up'] = c.num_cells_up
                if d > 0:
                    kw['num_cells_down'] = c.num_cells_down
                x = c.x.float() + 0.5 * torch.randn(c.x.shape, generator=gen)
                cochains.append(RefCochain(dim=d, x=x, num_cells=c.num_cells, **kw))
            out.append(RefComplex(*cochains, dimension=cx.dimension))
    return out


class Inputs:
    """The complexes of every input kind, drawn once; `batch(kind, dtype)` collates a fresh reference batch (the models write x
    back into the batch they are given)."""

    def __init__(self):
        gen = torch.Generator().manual_seed(2024)
        self.complexes = {k: mol_complexes(k, gen) for k in ('mol', 'ogb', 'mol_noedge', 'nodes_only')}
        self.complexes['sr'] = sr_complexes(gen)

    def batch(self, kind, dtype=torch.float32):
        b = RefBatch.from_complex_list(copy.deepcopy(self.complexes[kind]), max_dim=2)
        if kind == 'sr':
            for d in range(b.dimension + 1):
                b.cochains[d].x = b.cochains[d].x.to(dtype)
        return b


def graph_inputs():
    """index_like_oriented(130, 7) over vertices 0..129, cut into 4 graphs by a sorted batch vector, plus 3 vertices without
    edges as graph 4; a mask of one vertex per graph; features per width drawn on demand (seeded by the width)."""
    index = index_like_oriented(130, 7)
    batch = torch.cat([torch.repeat_interleave(torch.arange(4), torch.tensor([40, 25, 35, 30])), torch.full((3,), 4)])
    mask = torch.zeros(133, dtype=torch.bool)
    mask[[3, 41, 70, 129, 131]] = True
    deg = torch.bincount(index[1], minlength=133)
    assert {0, 64, 65, 300} <= set(deg.tolist()) and int((deg == 0).sum()) >= 133 // 3
    return index, batch, mask


def graph_x(width):
    return torch.randn(133, width, generator=torch.Generator().manual_seed(100 + width))


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
def randomise(model, gen):
    """BatchNorm running statistics as oracle/gen_golden.py draws them; affine terms of every norm away from (1, 0); every
    trained eps away from 0 (distinct values: a mix-up of eps1 / eps2 / eps3 shows)."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(generator=gen)
                m.running_var.uniform_(0.5, 1.5, generator=gen)
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=gen))
        for n, p in model.named_parameters():
            if n.split('.')[-1].startswith('eps'):
                p.copy_(0.1 + 0.5 * torch.rand(1, generator=gen))
    return model


def in_float64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def hook_layers(modules, seen):
    """Forward hooks that record every module's output under 'layer{c}' (a tensor) or 'layer{c}_{k}' (a list, one per dimension)."""
    def make(c):
        def hook(mod, inp, res):
            if torch.is_tensor(res):
                seen[f'layer{c}'] = res
            else:
                for k, r in enumerate(res):
                    seen[f'layer{c}_{k}'] = r
        return hook
    return [m.register_forward_hook(make(c)) for c, m in enumerate(modules)]


def run_cell(model, batch):
    """-> (out, {name: partial})."""
    if isinstance(model, RMM.EmbedSparseCINNoRings):
        seen = {}
        hooks = hook_layers(model.convs, seen)
        out = model(batch)
        for h in hooks:
            h.remove()
        return out, seen
    out, res = model(batch, include_partial=True)
    return out, {k: v for k, v in res.items() if k != 'out'}


def run_graph(model, data):
    seen = {}
    hooks = hook_layers([model.conv1] + list(model.convs) if hasattr(model, 'conv1') else list(model.convs), seen)
    out = model(data)
    for h in hooks:
        h.remove()
    return out, seen


def store(out, case, model, run32, run64):
    """State, both runs, and the condition on the inputs."""
    model.eval()
    for k, v in model.state_dict().items():
        out[f'{case}/state/{k}'] = G.np_(v)
    with torch.no_grad():
        y32, p32 = run32(model)
        m64 = copy.deepcopy(model).double()
        y64, p64 = in_float64(lambda: run64(m64))
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and set(p32) == set(p64) and p64, case
    worst = 0.0
    for name, t32, t64 in [('out', y32, y64)] + [(k, p32[k], p64[k]) for k in p64]:
        assert t64.dtype == torch.float64 and t32.dtype == torch.float32, (case, name)
        err = float((t32.double() - t64).abs().max())
        bound = HALF_GATE * max(1.0, float(t64.abs().max()))
        assert err <= bound, f'{case} {name}: the reference in float32 is {err:.3e} from float64, above {bound:.3e}'
        worst = max(worst, err / bound)
    print(f'{case}: float32 reference within {worst:.2f} of half the gate')
    out[f'{case}/out64'], out[f'{case}/out32'] = G.np_(y64), G.np_(y32)
    for k in p64:                   # (the float32 partials were held to the condition above; only the float64 ones are kept)
        out[f'{case}/p64/{k}'] = G.np_(p64[k])


def train_part(out, case, model, run, gen):
    """float64, train() mode: output, cotangent, every parameter's gradient; and how far the reference's own float32 autograd
    is from them."""
    def grads(m, dtype):
        m.train()
        y, _ = run(m, dtype)
        c = cot.to(dtype)
        (y * c).sum().backward()
        return y.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    m64 = copy.deepcopy(model).double()
    cot = None
    torch.set_default_dtype(torch.float64)
    try:
        m64.train()
        shape = run(copy.deepcopy(m64), torch.float64)[0].shape
        cot = torch.randn(shape, generator=gen, dtype=torch.float32).double()
        y64, g64 = grads(m64, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    y32, g32 = grads(copy.deepcopy(model), torch.float32)
    out[f'train/{case}/out'], out[f'train/{case}/cotangent'] = G.np_(y64), G.np_(cot)
    out[f'train/{case}/out32_err'] = np.float64(float((y32.double() - y64).abs().max()))
    for k, g in g64.items():
        out[f'train/{case}/grad/{k}'] = G.np_(g)
        out[f'train/{case}/grad32_err/{k}'] = np.float64(float((g32[k].double() - g).abs().max()))


# ------------------------------------------------------------------------------------------------
# the two fixtures
# ------------------------------------------------------------------------------------------------
def generate_cell(inputs):
    out = {}
    for kind in ('mol', 'ogb', 'sr'):
        G.dump_complex(out, f'inputs/{kind}', inputs.batch(kind))
    out['inputs/mol/names'] = np.array(G.MOL_LIST)
    gen = torch.Generator().manual_seed(11)
    for i, (case, (cls, args, kw, kind)) in enumerate(CELL_CASES.items()):
        torch.manual_seed(300 + i)
        model = randomise(getattr(RM if cls == 'SparseCIN' else RMM, cls)(*args, **kw), gen)
        out[f'{case}/cfg'] = np.array(json.dumps(dict(cls=cls, args=args, kw=kw, inputs=kind), sort_keys=True))
        store(out, case, model, lambda m: run_cell(m, inputs.batch(kind)), lambda m: run_cell(m, inputs.batch(kind, torch.float64)))
        if case in TRAIN_CASES:
            train_part(out, case, model, lambda m, dtype: run_cell(m, inputs.batch(kind, dtype)), gen)
    return out


def generate_gin(inputs):
    out = {}
    index, batch, mask = graph_inputs()
    out['graph/edge_index'], out['graph/batch'], out['graph/mask'] = G.np_(index), G.np_(batch), G.np_(mask)
    for kind in ('mol', 'mol_noedge', 'nodes_only'):
        G.dump_complex(out, f'inputs/{kind}', inputs.batch(kind))
    out['inputs/mol/names'], out['inputs/nodes_only/names'] = np.array(G.MOL_LIST), np.array(NODES_ONLY)
    gen = torch.Generator().manual_seed(12)
    for i, (case, (cls, args, kw)) in enumerate(GIN_CASES.items()):
        torch.manual_seed(400 + i)
        model = randomise(getattr(RRM if cls == 'RingGIN' else RGM, cls)(*args, **kw), gen)
        out[f'{case}/cfg'] = np.array(json.dumps(dict(cls=cls, args=args, kw=kw), sort_keys=True))
        x = graph_x(args[0])
        out[f'graph/x/{args[0]}'] = G.np_(x)

        def data(dtype):
            return SimpleNamespace(x=x.to(dtype), edge_index=index, batch=batch, mask=mask)
        store(out, case, model, lambda m: run_graph(m, data(torch.float32)), lambda m: run_graph(m, data(torch.float64)))
        if case in TRAIN_CASES:
            train_part(out, case, model, lambda m, dtype: run_graph(m, data(dtype)), gen)
    for i, (case, (args, kw, kind)) in enumerate(EGIN_CASES.items()):
        torch.manual_seed(500 + i)
        model = randomise(RMM.EmbedGIN(*args, **kw), gen)
        out[f'{case}/cfg'] = np.array(json.dumps(dict(cls='EmbedGIN', args=args, kw=kw, inputs=kind), sort_keys=True))
        store(out, case, model, lambda m: run_graph(m, inputs.batch(kind)), lambda m: run_graph(m, inputs.batch(kind)))
    return out


def main():
    check_gin_known_answers()
    G.check_reference_known_answers()
    inputs = Inputs()
    made = {CELL: generate_cell(inputs), GIN: generate_gin(inputs)}
    if '--check' in sys.argv[1:]:
        from tests._golden import load
        for name, out in made.items():
            have = load(name)
            assert set(have) == set(out), set(have) ^ set(out)
            for k in out:
                a, b = np.asarray(out[k]), np.asarray(have[k])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
            print(f'{name}: {len(out)} arrays regenerate bit-exactly')
        return
    for name, out in made.items():
        G.save(name, out)


if __name__ == '__main__':
    main()
