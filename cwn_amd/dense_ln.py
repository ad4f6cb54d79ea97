"""The update / combine networks of a layer built with graph_norm='ln' (mp/nn.py:39-47; the reference's cwn-csl.sh) as
grouped launches: per stage depth ONE grouped GEMM over every dimension and branch (ops.gemm_many, plain bias epilogue)
and ONE LayerNorm + ReLU launch (ops.layer_norm_act_many, csrc/cwn_layernorm.hip), forward and backward.

LayerNorm normalises every ROW, so unlike BatchNorm it cannot be folded into the per-column prologue / epilogue of the
GEMMs (layers._fold_norm, dense_train): it is a launch of its own behind each GEMM.  For a three-dimension SparseCINConv
that is 6 launches forward instead of the 45 of the torch modules (15 Linear, 15 native_layer_norm, 15 ReLU).  LayerNorm has
no mode, so the same code serves inference and training; autograd sees two Functions per stage.
"""
import os
from typing import List, Sequence

import torch
from torch import Tensor
from torch.nn import LayerNorm, Linear

from . import _ffi, ops

# False (CWN_FUSED_LN=0): LayerNorm layers run their networks as torch modules, one dimension and one branch at a time
FUSED_LN = os.environ.get('CWN_FUSED_LN') != '0'


def _stage_ok(stage) -> bool:
    lin, norm = stage
    return (isinstance(lin, Linear) and isinstance(norm, LayerNorm)
            and tuple(norm.normalized_shape) == (lin.out_features,) and lin.out_features <= _ffi.LN_MAX_N)


def supported(chains, combine) -> bool:
    """chains[dim][branch] and combine[dim] are what layers._mlp_stages returns for the update networks and the combine
    network: [(Linear, norm), ...] of Linear -> norm -> ReLU groups, or None.  True when every norm is a LayerNorm over
    exactly its Linear's outputs, every update network has the same depth, every dimension the same number of branches
    and every combine network is one stage."""
    if not chains or len(chains) != len(combine):
        return False
    nb = len(chains[0])
    if nb < 1 or any(len(branches) != nb for branches in chains):
        return False
    flat = [st for branches in chains for st in branches]
    if any(st is None or len(st) == 0 for st in flat) or len({len(st) for st in flat}) != 1:
        return False
    if any(cb is None or len(cb) != 1 for cb in combine):
        return False
    if not all(_stage_ok(s) for st in flat + list(combine) for s in st):
        return False
    # (the update stages are cwn_gemm_f32 launches: the whole K of a weight tile is resident in LDS)
    return all(lin.in_features <= ops.GEMM_MAX_K for st in flat for lin, _ in st)


def counted(chains, combine) -> bool:
    """Does every launch `run` makes for these networks carry the device-side row count of a static batch -- in the
    backward too?  True when `supported` accepts them and the combine product is a grouped GEMM or ops.linear_wide.  The
    torch branch (three / four branches: CIN++; a combine beyond cwn_linear_wide_f32) sums its weight gradient over the
    CAPACITY rows of a slot, and so do the torch modules a layer runs when `supported` declines or FUSED_LN is off."""
    if not FUSED_LN or not supported(chains, combine) or len(chains[0]) != 2:
        return False
    for branches, cb in zip(chains, combine):
        lin = cb[0][0]
        k1, k2 = (st[-1][0].out_features for st in branches)
        if k1 + k2 != lin.in_features or not ((lin.in_features <= ops.GEMM_MAX_K and k1 % 4 == 0)
                                              or ops.linear_wide_applies(k1, k2, lin.out_features)):
            return False
    return True


def run(chains, combine, outs: Sequence[Tensor]) -> List[Tensor]:
    """The networks `supported` accepted on `outs` ([dim][branch] flattened: the aggregated streams of every dimension);
    returns one matrix per dimension."""
    nd, nb = len(chains), len(chains[0])
    flat = [st for branches in chains for st in branches]
    hs = list(outs)
    for s in range(len(flat[0])):
        ys = ops.gemm_many([ops.Gemm(X=h, W=st[s][0].weight, bias=st[s][0].bias) for h, st in zip(hs, flat)])
        hs = ops.layer_norm_act_many(ys, [st[s][1] for st in flat], relu=True)
    lins = [cb[0][0] for cb in combine]
    if nb == 2 and all(lin.in_features <= ops.GEMM_MAX_K and hs[2 * i].size(1) % 4 == 0 for i, lin in enumerate(lins)):
        # torch.cat folded into the K-concatenation of the GEMM (cwn_gemm_f32 wants K % 4 == 0 next to X2)
        ys = ops.gemm_many([ops.Gemm(X=hs[2 * i], X2=hs[2 * i + 1], W=lin.weight, bias=lin.bias) for i, lin in enumerate(lins)])
    elif nb == 2 and all(ops.linear_wide_applies(hs[2 * i].size(1), hs[2 * i + 1].size(1), lin.out_features)
                         for i, lin in enumerate(lins)):
        # wider than the GEMM's K (width 160: 320) or a width that is no multiple of 4: K streamed (csrc/cwn_linear_wide.hip),
        # under the row count of a static batch
        ys = [ops.linear_wide(hs[2 * i], hs[2 * i + 1], lin.weight, lin.bias) for i, lin in enumerate(lins)]
    else:
        # three / four branches (CIN++), or beyond cwn_linear_wide_f32 (N > 256, K + K2 > 512): the torch modules
        ys = [torch.nn.functional.linear(torch.cat(hs[nb * i: nb * (i + 1)], dim=-1), lin.weight, lin.bias)
              for i, lin in enumerate(lins)]
    return ops.layer_norm_act_many(ys, [cb[0][1] for cb in combine], relu=True)
