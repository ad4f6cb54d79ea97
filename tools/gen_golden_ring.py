"""tests/golden/ring_sparse_cin.npz: the reference's RingSparseCIN (mp/ring_exp_models.py) run on the ring-transfer complexes.

    python tools/gen_golden_ring.py            # write the fixture
    python tools/gen_golden_ring.py --check    # regenerate in memory and compare with the committed file, array by array

CPU only.  The reference is imported behind the stand-ins of oracle/refshim exactly as oracle/gen_golden.py imports it (that
module is read, not changed: its path setup, `np_` and `save` are used from here); its batches are built by the reference's own
data/complex.py classes -- which collate the extra `mask` key -- from the arrays of cwn_amd.synthetic.ring_transfer.  The per-graph
arrays (x, y, the ring lift's index tensors) therefore come from THIS project's generator and lift: the fixture does not pin them
against the reference's own lift (data/utils.py needs graph-tool); what is reference-made is the batching, the `mask` collation
and every model output.  What is
written is data: inputs, the batched index tensors and `mask`, one state_dict, logits and every `layer{c}_{k}` partial output.

Cases: rings of 4, 10 and 30 vertices (five complexes each, one per class) and one batch that mixes rings of 10 and 30;
use_coboundaries on and off; hidden 64, 3 layers, eval mode.  The model without co-boundaries has a subset of the other's
parameters: one state_dict ('state/...') serves both.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402  (puts oracle/refshim and the reference on sys.path)
from data.complex import Cochain as RefCochain, Complex as RefComplex, ComplexBatch as RefBatch  # noqa: E402
from mp.ring_exp_models import RingSparseCIN as RefRingSparseCIN  # noqa: E402

from cwn_amd import synthetic  # noqa: E402

NAME = 'ring_sparse_cin.npz'
CLASSES, HIDDEN, LAYERS = 5, 64, 3
INDEX_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')


def cases():
    """name -> the complexes (cwn_amd containers) of the batch."""
    r4, r10, r30 = (synthetic.ring_transfer(n, CLASSES, CLASSES) for n in (4, 10, 30))
    return {'ring4': r4, 'ring10': r10, 'ring30': r30, 'mixed': [r10[1], r30[3], r30[0], r10[4]]}


def to_reference(cx):
    """The same complex in the reference's containers (fresh tensors: its model writes x back)."""
    cochains = []
    for d in range(cx.dimension + 1):
        c = cx.cochains[d]
        kw = {k: c[k].clone() for k in INDEX_KEYS if c[k] is not None}
        if d == 0:
            kw['mask'] = c.mask.clone()
        kw['num_cells_up'] = c.num_cells_up
        if d > 0:
            kw['num_cells_down'] = c.num_cells_down
        cochains.append(RefCochain(dim=d, x=c.x.clone(), num_cells=c.num_cells, **kw))
    return RefComplex(*cochains, y=cx.y.clone(), dimension=cx.dimension)


def generate():
    torch.manual_seed(20)
    out = {}
    models = {}
    models['cob1'] = RefRingSparseCIN(CLASSES, CLASSES, LAYERS, HIDDEN, use_coboundaries=True).eval()
    models['cob0'] = RefRingSparseCIN(CLASSES, CLASSES, LAYERS, HIDDEN, use_coboundaries=False).eval()
    full = models['cob1'].state_dict()
    assert set(models['cob0'].state_dict()) <= set(full)
    models['cob0'].load_state_dict({k: full[k] for k in models['cob0'].state_dict()})
    for k, v in full.items():
        out[f'state/{k}'] = G.np_(v)
    out['state_keys/cob0'] = np.array(sorted(models['cob0'].state_dict()))
    out['state_keys/cob1'] = np.array(sorted(full))
    for name, complexes in cases().items():
        for i, cx in enumerate(complexes):
            out[f'{name}/graphs/{i}/x'] = G.np_(cx.nodes.x)
            out[f'{name}/graphs/{i}/y'] = G.np_(cx.y)
            out[f'{name}/graphs/{i}/nodes'] = np.int64(cx.nodes.num_cells)
        for tag, model in models.items():
            batch = RefBatch.from_complex_list([to_reference(cx) for cx in complexes], max_dim=2)
            if tag == 'cob1':
                for d in range(3):
                    c = batch.cochains[d]
                    out[f'{name}/batch/{d}/x'] = G.np_(c.x)
                    out[f'{name}/batch/{d}/batch'] = G.np_(c.batch)
                    for k in INDEX_KEYS:
                        if c[k] is not None:
                            out[f'{name}/batch/{d}/{k}'] = G.np_(c[k])
                out[f'{name}/batch/0/mask'] = G.np_(batch.nodes.mask)
                out[f'{name}/batch/y'] = G.np_(batch.y)
            with torch.no_grad():
                logits, res = model(batch, include_partial=True)
            out[f'{name}/{tag}/out'] = G.np_(logits)
            for k, v in res.items():
                if k != 'out':
                    out[f'{name}/{tag}/{k}'] = G.np_(v)
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
