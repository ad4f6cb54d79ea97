"""tests/golden/mp_agnostic.npz: the reference's MessagePassingAgnostic (mp/models.py:618-661) -- the control of the
strongly-regular-graph experiment (exp/scripts/cwn-sr-base.sh) -- run on batches built by the reference's own containers.

    python tools/gen_golden_agnostic.py            # write the fixture
    python tools/gen_golden_agnostic.py --check    # regenerate in memory and compare with the committed file, array by array

CPU only.  The reference is imported behind the stand-ins of oracle/refshim exactly as oracle/gen_golden.py imports it (that
module is read, not changed: its path setup, `get`, `np_` and `save` are used from here).  The dummy complexes are the
reference's (data/dummy_complexes.py: the ones tests/golden/dummy_complexes.npz holds); the SR(16,6,2,2) lifts come from THIS
project's generator and lift (cwn_amd.synthetic.sr_lift) and are batched by the reference's data/complex.py classes.  What is
written is data: the batched inputs (x and the batch vector per dimension), one state_dict, and per configuration the input
of lin1 -- the per-dimension pooled rows [max_dim + 1, C, H], rows of an absent dimension zero -- and the logits.

Cases: 'dummy_mixed' (complexes with and without 2-cells), 'dummy_no2' (no complex has a 2-cell: the batch has two
dimensions, the model three), 'sr3' and 'sr6' (the rook's graph, the Shrikhande graph and a relabelled copy of each, rings up to
3 / 6).  Configurations: elu | relu  x  sum | mean  x  float32 | float64; hidden 32, 8 classes, eval mode.  The parameters are
drawn once in float64 ('state/...'); the float32 models load them rounded to float32.  The reference allocates its pooled
matrix in the default dtype, so each dtype runs under torch.set_default_dtype, as exp/run_sr_exp.py does for float64.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402  (puts oracle/refshim and the reference on sys.path)
from data.complex import Cochain as RefCochain, Complex as RefComplex, ComplexBatch as RefBatch  # noqa: E402
from mp.models import MessagePassingAgnostic as RefAgnostic  # noqa: E402

from cwn_amd import synthetic  # noqa: E402

NAME = 'mp_agnostic.npz'
HIDDEN, CLASSES, MAX_DIM = 32, 8, 2
DUMMY = {'dummy_mixed': ['house', 'fullstop', 'kite', 'square', 'colon', 'filled_square', 'molecular'],
         'dummy_no2': ['square', 'colon', 'fullstop', 'square_dot']}
SR_RINGS = {'sr3': 3, 'sr6': 6}
ACTS, READOUTS = ('elu', 'relu'), ('sum', 'mean')
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
INDEX_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')


def sr_complexes(max_k):
    """The rook's graph, a relabelled copy, the Shrikhande graph, a relabelled copy (cwn_amd containers, float64)."""
    rng = np.random.default_rng(43)
    out = []
    for g in (synthetic.rook_4x4(), synthetic.shrikhande()):
        out += [synthetic.sr_lift(*g, max_k=max_k), synthetic.sr_lift(*synthetic.relabel(*g, rng.permutation(16)), max_k=max_k)]
    return out


def to_reference(cx):
    """The same complex in the reference's containers."""
    cochains = []
    for d in range(cx.dimension + 1):
        c = cx.cochains[d]
        kw = {k: c[k].clone() for k in INDEX_KEYS if c[k] is not None}
        kw['num_cells_up'] = c.num_cells_up
        if d > 0:
            kw['num_cells_down'] = c.num_cells_down
        cochains.append(RefCochain(dim=d, x=c.x.clone(), num_cells=c.num_cells, **kw))
    return RefComplex(*cochains, dimension=cx.dimension)


def batch_of(case, dtype):
    """A fresh reference batch of `case` with features in `dtype`."""
    if case in DUMMY:
        complexes = [G.get(n) for n in DUMMY[case]]
    else:
        complexes = [to_reference(cx) for cx in sr_complexes(SR_RINGS[case])]
    batch = RefBatch.from_complex_list(complexes, max_dim=MAX_DIM)
    for d in range(batch.dimension + 1):
        batch.cochains[d].x = batch.cochains[d].x.to(dtype)
    return batch


def generate():
    out = {}
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(21)
    state = RefAgnostic(1, CLASSES, HIDDEN, dropout_rate=0.5, max_dim=MAX_DIM, nonlinearity='elu', readout='sum').state_dict()
    for k, v in state.items():
        out[f'state/{k}'] = G.np_(v)
    out['state_keys'] = np.array(sorted(state))
    for case, names in DUMMY.items():
        out[f'{case}/names'] = np.array(names)
    try:
        for tag, dtype in DTYPES.items():
            torch.set_default_dtype(dtype)
            for case in list(DUMMY) + list(SR_RINGS):
                batch = batch_of(case, dtype)
                if tag == 'f64':
                    out[f'{case}/dimension'] = np.int64(batch.dimension)
                    for d in range(batch.dimension + 1):
                        out[f'{case}/batch/{d}/x'] = G.np_(batch.cochains[d].x)
                        out[f'{case}/batch/{d}/batch'] = G.np_(batch.cochains[d].batch)
                for act in ACTS:
                    for readout in READOUTS:
                        model = RefAgnostic(1, CLASSES, HIDDEN, dropout_rate=0.5, max_dim=MAX_DIM, nonlinearity=act,
                                            readout=readout).eval()
                        model.load_state_dict({k: v.to(dtype) for k, v in state.items()})
                        seen = []
                        hook = model.lin1.register_forward_hook(lambda mod, inp, res: seen.append(inp[0]))
                        with torch.no_grad():
                            logits = model(batch_of(case, dtype))
                        hook.remove()
                        assert len(seen) == 1 and seen[0].dtype == dtype and logits.dtype == dtype
                        out[f'{case}/{act}/{readout}/{tag}/pooled'] = G.np_(seen[0])
                        out[f'{case}/{act}/{readout}/{tag}/out'] = G.np_(logits)
    finally:
        torch.set_default_dtype(torch.float32)
    return out


def main():
    out = generate()
    if '--check' in sys.argv[1:]:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from tests._golden import load
        have = load(NAME)
        assert set(have) == set(out), set(have) ^ set(out)
        for k in out:
            a, b = np.asarray(out[k]), np.asarray(have[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        print(f'{NAME}: {len(out)} arrays regenerate bit-exactly')
        return
    G.save(NAME, out)


if __name__ == '__main__':
    main()
