"""The control of the strongly-regular-graph isomorphism experiment (exp/scripts/cwn-sr-base.sh, mpsn-sr-base.sh; the other
half is examples/sr_isomorphism.py): an UNTRAINED MessagePassingAgnostic (mp/models.py:618-661; hidden 256, ELU, sum
readout, float64) -- no message passing, a Linear and the nonlinearity per cell, the readout per dimension, two more Linear
layers -- embeds the ring lift of the two graphs of SR(16, 6, 2, 2) and of a vertex-relabelled copy of each, for rings up to
3, 4, 5 and 6, and the reference's criterion (exp/test_sr.py:82: two complexes are taken for isomorphic when their
embeddings are within 0.01, torch.pdist) is read at each ring size.

What the control can see is how many cells of each size a lift has, nothing else.  At rings up to 3 both graphs lift to
16 / 48 / 32 cells with identical features, so it embeds them identically and fails to tell them apart; from rings up to 4
on the numbers of 2-cells differ (68 against 44 at 4, 164 against 204 at 6) and it tells them apart by counting -- the
figure SparseCIN's are read against.

In inference the forward is two launches of csrc/cwn_agnostic.hip (embed + activate + pool for all dimensions; the head);
CWN_FUSED_AGNOSTIC=0 puts it back on torch.nn.Linear (rocBLAS dgemm) and the segmented-reduce kernel.

    python examples/sr_baseline.py [seed]        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd.complex import ComplexBatch                                   # noqa: E402
from cwn_amd.models import MessagePassingAgnostic                          # noqa: E402
from cwn_amd.synthetic import relabel, rook_4x4, shrikhande, sr_lift       # noqa: E402

EPS = 0.01                   # the reference's criterion (exp/test_sr.py:82)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device('cuda', 0)
    torch.set_default_dtype(torch.float64)
    graphs = {'rook 4x4': rook_4x4(), 'Shrikhande': shrikhande()}
    torch.manual_seed(seed)
    model = MessagePassingAgnostic(num_input_features=1, num_classes=16, hidden=256, dropout_rate=0.0, max_dim=2,
                                   nonlinearity='elu', readout='sum').to(dev).eval()
    for max_k in (3, 4, 5, 6):
        rng = np.random.default_rng(43)
        batch, names = [], []
        for name, g in graphs.items():
            batch += [sr_lift(*g, max_k=max_k), sr_lift(*relabel(*g, rng.permutation(16)), max_k=max_k)]
            names += [name, name + ' (relabelled)']
        cells = [[cx.cochains[d].num_cells if d <= cx.dimension else 0 for d in range(3)] for cx in (batch[0], batch[2])]
        with torch.no_grad():
            emb = model(ComplexBatch.from_complex_list(batch, max_dim=2).to(dev))
        print(f'rings up to {max_k}: cells {cells[0]} against {cells[1]}; embeddings {tuple(emb.shape)} {emb.dtype} '
              f'({model.last_route} route)')
        for i in (0, 2):
            d = float(torch.pdist(emb[i:i + 2], p=2))
            print(f'  {names[i]:<12} vs its relabelled copy: {d:.3e}  ({"isomorphic: within" if d <= EPS else "ABOVE"} {EPS})')
        d = float(torch.pdist(emb[[0, 2]], p=2))
        print(f'  rook 4x4 vs Shrikhande:              {d:.3e}  ({"told apart" if d > EPS else "NOT told apart"})')


if __name__ == '__main__':
    main()
