"""What the MessagePassingAgnostic tests share: the cases of tests/golden/mp_agnostic.npz (tools/gen_golden_agnostic.py) as
product-side batches, and the mirror loaded with the fixture's state."""
import numpy as np
import torch

from cwn_amd import synthetic
from cwn_amd.complex import ComplexBatch
from cwn_amd.models import MessagePassingAgnostic
from tests._golden import load, state_dict
from tests._product import dummy_complex

G = 'mp_agnostic.npz'
CASES = ('dummy_mixed', 'dummy_no2', 'sr3', 'sr6')
SR_RINGS = {'sr3': 3, 'sr6': 6}
CONFIGS = [(act, readout) for act in ('elu', 'relu') for readout in ('sum', 'mean')]
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}      # the project's gates: tests/_product.py, tests/test_gpu_f64_dense.py


def sr_complexes(max_k, dtype=torch.float64):
    """The rook's graph, a relabelled copy, the Shrikhande graph, a relabelled copy -- the generator's order and permutations."""
    rng = np.random.default_rng(43)
    out = []
    for g in (synthetic.rook_4x4(), synthetic.shrikhande()):
        out += [synthetic.sr_lift(*g, max_k=max_k, dtype=dtype),
                synthetic.sr_lift(*synthetic.relabel(*g, rng.permutation(16)), max_k=max_k, dtype=dtype)]
    return out


def case_complexes(case, dtype):
    if case in SR_RINGS:
        return sr_complexes(SR_RINGS[case], dtype)
    complexes = [dummy_complex(str(n)) for n in load(G)[f'{case}/names']]
    for cx in complexes:
        for d in range(cx.dimension + 1):
            cx.cochains[d].x = cx.cochains[d].x.to(dtype)
    return complexes


def case_batch(case, dtype, device=None):
    """A fresh batch of `case` with features in `dtype`."""
    b = ComplexBatch.from_complex_list(case_complexes(case, dtype), max_dim=2)
    return b.to(device) if device is not None else b


def fixture_model(act, readout, dtype, device=None, hidden=32, classes=8, dropout_rate=0.5):
    """The mirror in eval mode with the fixture's parameters (drawn in float64; a float32 model loads them rounded)."""
    model = MessagePassingAgnostic(1, classes, hidden, dropout_rate=dropout_rate, max_dim=2, nonlinearity=act, readout=readout)
    model = model.to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in state_dict(load(G), 'state').items()})
    model = model.eval()
    return model.to(device) if device is not None else model
