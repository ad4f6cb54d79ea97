"""The operand checks of linear_many_f64, update_chain_f64, embed_pool, agnostic_head and gin_layer: exception type and the
whole message, as literals recorded from the commit before the ops shared one checker (ops._rows_operand).  What is
reachable without a GPU: a wrong dtype, a non-tensor, mixed dtypes in one agnostic call, a CPU tensor of the right dtype.
The shape / stride clause needs a GPU tensor: tests/test_gpu_f64_dense.py, test_gpu_agnostic.py, test_gpu_gin.py."""
import pytest
import torch

from cwn_amd import ops

F16, F32, F64 = torch.float16, torch.float32, torch.float64

_F64_HINT = ': this kernel computes in fp64 only (float32 runs through the MFMA launches: gemm_many, update_mlp)'
_AGN_HINT = ': the kernels of csrc/cwn_agnostic.hip compute in fp32 or fp64 only'
_GIN_HINT = (': cwn_gin_layer_f32 computes in fp32 only (float64 and training run through ops.aggregate and the torch modules: '
             'layers.GINConv)')


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


def _linear(x):
    return lambda: ops.linear_many_f64([(x, z(2, 4, dtype=F64), z(2, dtype=F64), 'id')])


def _chain(**over):
    F, H, n = 3, 4, 5
    d = lambda *s: z(*s, dtype=F64)
    kw = dict(in_up=d(n, F), in_b=d(n, F), weights=[d(H, F), d(H, H), d(H, F), d(H, H), d(H, 2 * H)],
              biases=[d(H) for _ in range(5)], folds=[(d(H), d(H)) for _ in range(5)], act='relu', out=None)
    kw.update(over)
    return lambda: ops.update_chain_f64([ops.ChainDim(**kw)])


def _embed(x, w, b):
    return lambda: ops.embed_pool([x], [torch.tensor([0, 4])], 1, [w], [b], 'elu')


def _head(p, w1, b1, w2, b2):
    return lambda: ops.agnostic_head([p], w1, b1, w2, b2, 'elu')


def _gin(x):
    return lambda: ops.gin_layer(x, None, None, [(z(5, 3), None, None, None), (z(5, 5), None, None, None)], 'relu')


CASES = {
    'linear.float16': (_linear(z(3, 4, dtype=F16)), TypeError, 'x[0] must be float64 (got torch.float16)' + _F64_HINT),
    'linear.float32': (_linear(z(3, 4)), TypeError, 'x[0] must be float64 (got torch.float32)' + _F64_HINT),
    'linear.list': (_linear([[0.0] * 4] * 3), TypeError, 'x[0] must be float64 (got list)' + _F64_HINT),
    'linear.cpu': (_linear(z(3, 4, dtype=F64)), TypeError, 'x[0] must be a float64 tensor on the GPU (got torch.float64 on cpu)'),
    'chain.float16': (_chain(in_up=z(5, 3, dtype=F16)), TypeError, 'dims[0].in_up must be float64 (got torch.float16)' + _F64_HINT),
    'chain.float32': (_chain(in_up=z(5, 3)), TypeError, 'dims[0].in_up must be float64 (got torch.float32)' + _F64_HINT),
    'chain.list': (_chain(in_up=[[0.0] * 3] * 5), TypeError, 'dims[0].in_up must be float64 (got list)' + _F64_HINT),
    'chain.cpu': (_chain(), TypeError, 'dims[0].in_up must be a float64 tensor on the GPU (got torch.float64 on cpu)'),
    'embed.float16': (_embed(z(4, 3, dtype=F16), z(8, 3, dtype=F16), z(8, dtype=F16)), TypeError,
                      'embed_pool: xs[0] must be float32 or float64 (got torch.float16)' + _AGN_HINT),
    'embed.list': (_embed(z(4, 3), [[0.0] * 3] * 8, z(8)), TypeError,
                   'embed_pool: weights[0] must be float32 or float64 (got list)' + _AGN_HINT),
    'embed.mixed.float64': (_embed(z(4, 3), z(8, 3, dtype=F64), z(8)), TypeError,
                            'embed_pool: weights[0] is torch.float64, the operands before it torch.float32: all operands of a '
                            'call share one dtype'),
    'embed.mixed.float32': (_embed(z(4, 3, dtype=F64), z(8, 3, dtype=F64), z(8)), TypeError,
                            'embed_pool: biases[0] is torch.float32, the operands before it torch.float64: all operands of a '
                            'call share one dtype'),
    # the dtypes of ALL operands are checked before the device of the first: a float16 bias behind CPU operands is named
    'embed.float16.last': (_embed(z(4, 3), z(8, 3), z(8, dtype=F16)), TypeError,
                           'embed_pool: biases[0] must be float32 or float64 (got torch.float16)' + _AGN_HINT),
    'embed.cpu.float32': (_embed(z(4, 3), z(8, 3), z(8)), TypeError,
                          'embed_pool: xs[0] must be a torch.float32 tensor on the GPU (it is on cpu)'),
    'embed.cpu.float64': (_embed(z(4, 3, dtype=F64), z(8, 3, dtype=F64), z(8, dtype=F64)), TypeError,
                          'embed_pool: xs[0] must be a torch.float64 tensor on the GPU (it is on cpu)'),
    'head.float16': (_head(z(1, 8, dtype=F16), z(8, 8, dtype=F16), None, z(2, 8, dtype=F16), None), TypeError,
                     'agnostic_head: pooled[0] must be float32 or float64 (got torch.float16)' + _AGN_HINT),
    'head.list': (_head(z(1, 8), z(8, 8), [0.0] * 8, z(2, 8), z(2)), TypeError,
                  'agnostic_head: lin1_b must be float32 or float64 (got list)' + _AGN_HINT),
    'head.mixed.float64': (_head(z(1, 8), z(8, 8), z(8), z(2, 8, dtype=F64), z(2)), TypeError,
                           'agnostic_head: lin2_w is torch.float64, the operands before it torch.float32: all operands of a '
                           'call share one dtype'),
    'head.mixed.float32': (_head(z(1, 8, dtype=F64), z(8, 8, dtype=F64), z(8), z(2, 8, dtype=F64), None), TypeError,
                           'agnostic_head: lin1_b is torch.float32, the operands before it torch.float64: all operands of a '
                           'call share one dtype'),
    'head.cpu.float32': (_head(z(1, 8), z(8, 8), z(8), z(2, 8), z(2)), TypeError,
                         'agnostic_head: pooled[0] must be a torch.float32 tensor on the GPU (it is on cpu)'),
    'head.cpu.float64': (_head(z(1, 8, dtype=F64), z(8, 8, dtype=F64), None, z(2, 8, dtype=F64), None), TypeError,
                         'agnostic_head: pooled[0] must be a torch.float64 tensor on the GPU (it is on cpu)'),
    'gin.float16': (_gin(z(4, 3, dtype=F16)), TypeError, 'gin_layer: x must be float32 (got torch.float16)' + _GIN_HINT),
    'gin.float64': (_gin(z(4, 3, dtype=F64)), TypeError, 'gin_layer: x must be float32 (got torch.float64)' + _GIN_HINT),
    'gin.list': (_gin([[0.0] * 3] * 4), TypeError, 'gin_layer: x must be float32 (got list)' + _GIN_HINT),
    'gin.cpu': (_gin(z(4, 3)), TypeError, 'gin_layer: x must be a float32 tensor on the GPU (got torch.float32 on cpu)'),
    # oriented_layer resolves its activation like every other op: an unknown name lists the choices (it was a bare KeyError)
    'oriented.gelu': (lambda: ops.oriented_layer(z(4, 3), None, None, None, None, z(5, 3), None, None, act='gelu'), ValueError,
                      "unknown activation 'gelu': one of ['elu', 'id', 'relu', 'sigmoid', 'tanh'] or a CWN_ACT_* code"),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_exception_and_its_whole_message(case):
    call, exc, message = CASES[case]
    with pytest.raises(exc) as got:
        call()
    assert type(got.value) is exc and str(got.value) == message
