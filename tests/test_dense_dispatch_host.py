"""Host-side facts of a conv layer's dense dispatch (no GPU, no library call): which update networks `_update_chains` hands
out and in which order, when it declines, the order in which `forward` tries the `_dense_*` paths and what it does when all of
them decline, and what dense_train._Plan derives from its chains."""
from types import SimpleNamespace

import pytest
import torch
from torch.nn import BatchNorm1d as BN, ReLU

from cwn_amd import dense_train
from cwn_amd.layers import CINppConv, SparseCINConv

# (class, constructor switches, update networks of a level in the order of `outs`)
FORMS = [(SparseCINConv, {}, ('update_up_nn', 'update_boundaries_nn')),
         (CINppConv, {}, ('update_up_nn', 'update_down_nn', 'update_boundaries_nn')),
         (CINppConv, dict(coboundary_stream=True), ('update_up_nn', 'update_down_nn', 'update_boundaries_nn', 'update_coboundaries_nn'))]
IDS = ['cin', 'cinpp', 'cinpp-cob']


def _conv(cls=SparseCINConv, hidden=8, **kw):
    args = (hidden, hidden, hidden) + (None,) * (4 if cls is SparseCINConv else 6)
    return cls(*args, max_dim=2, hidden=hidden, act_module=ReLU, layer_dim=hidden, graph_norm=BN, use_coboundaries=True, **kw).eval()


def _plans(nb, n=3, start=0):
    return [None] * start + [[None] * nb for _ in range(start, n)]          # (a processed dimension: its nb streams)


@pytest.mark.parametrize('cls,kw,names', FORMS, ids=IDS)
@pytest.mark.parametrize('start', [0, 1, 2])
def test_update_chains_hands_out_the_networks_in_the_order_of_outs(cls, kw, names, start):
    conv, nb = _conv(cls, **kw), len(names)
    got = conv._update_chains(_plans(nb, start=start), [None] * (nb * (3 - start)), start)
    active, n_branches, chains = got[0], got[1], got[2]
    assert active == list(range(start, 3)) and n_branches == nb and len(chains) == 3 - start
    for d, branches in zip(active, chains):
        assert len(branches) == nb
        for name, stages in zip(names, branches):
            net = getattr(conv.mp_levels[d], name)
            assert len(stages) == 2 and stages[0][0] is net[0] and stages[1][0] is net[3]          # the Linear modules themselves
            assert stages[0][1] is net[1] and stages[1][1] is net[4]                                # ... and their norms
    if len(got) > 3:
        assert [cb[0][0] for cb in got[3]] == [conv.mp_levels[d].combine_nn[0] for d in active]
        assert all(len(cb) == 1 and cb[0][1] is conv.mp_levels[d].combine_nn[1] for d, cb in zip(active, got[3]))


@pytest.mark.parametrize('cls,kw,names', FORMS, ids=IDS)
def test_update_chains_declines(cls, kw, names):
    conv, nb = _conv(cls, **kw), len(names)
    plans = _plans(nb)
    assert conv._update_chains(plans, [None] * (3 * nb), 0) is not None
    assert conv._update_chains([plans[0], None, plans[2]], [None] * (3 * nb), 0) is None        # a dimension without streams
    assert conv._update_chains(plans, [None] * (3 * nb), 3) is None                               # nothing to process
    for n_outs in (3 * nb - 1, 3 * nb + 1, 2 * nb):
        assert conv._update_chains(plans, [None] * n_outs, 0) is None
    assert conv._update_chains(_plans(nb, start=1), [None] * (2 * nb), 0) is None               # (plans[0] is None below start 1)
    assert conv._update_chains(_plans(nb, start=1), [None] * (2 * nb), 1) is not None


def test_update_chains_declines_unequal_stream_counts():
    conv = _conv(CINppConv, coboundary_stream=True)
    plans = [[None] * 3, [None] * 4, [None] * 3]
    for n_outs in (9, 10, 12):
        assert conv._update_chains(plans, [None] * n_outs, 0) is None
    assert conv._update_chains(['blocked'] * 3, [None] * 9, 0)[1] == 3                            # (the blocked launch: three outputs)


def _stub(conv, plans, outs, answers):
    """`conv` with propagate_all, the `_dense_*` paths named in `answers` and every level's finish / forward_unfused replaced by
    recorders; returns the log."""
    log = []
    conv.propagate_all = lambda *params, start_to_process=0: (plans, outs)
    for name, answer in answers.items():
        def path(plans_, outs_, start=0, *rest, _name=name, _answer=answer):
            assert plans_ is plans and outs_ is outs
            log.append((_name, start))
            return _answer
        setattr(conv, name, path)
    for d, lvl in enumerate(conv.mp_levels):
        lvl.finish = lambda *xs, _d=d: (log.append(('finish', _d, xs)), ('finished', _d))[1]
        lvl.forward_unfused = lambda cochain, _d=d: (log.append(('unfused', _d, cochain)), ('unfused', _d))[1]
    return log


@pytest.mark.parametrize('cls,kw,names', FORMS, ids=IDS)
def test_forward_tries_the_dense_paths_in_order_and_stops_at_the_first(cls, kw, names):
    nb = len(names)
    # (CINppConv never reaches a float64 launch: its _dense_f64, if asked at all, declines by itself and stays as it is)
    order = ['_dense_eval', '_dense_f64', '_dense_train', '_dense_ln'] if cls is SparseCINConv else ['_dense_eval', '_dense_train', '_dense_ln']
    params = [SimpleNamespace(x=torch.zeros(2, 8)) for _ in range(3)]
    for start in (0, 1):
        plans, outs = _plans(nb, start=start), [torch.zeros(2, 8) for _ in range(nb * (3 - start))]
        for taker in range(len(order)):
            conv = _conv(cls, **kw)
            dense = [object() for _ in range(3 - start)]
            log = _stub(conv, plans, outs, {name: (dense if i == taker else None) for i, name in enumerate(order)})
            got = conv(*params, start_to_process=start)
            assert log == [(name, start) for name in order[:taker + 1]]
            assert all(g is p.x for g, p in zip(got[:start], params)) and all(g is h for g, h in zip(got[start:], dense))
            assert len(got) == 3


@pytest.mark.parametrize('cls,kw,names', FORMS, ids=IDS)
def test_forward_with_every_path_declining_runs_the_modules(cls, kw, names):
    nb = len(names)
    order = ['_dense_eval', '_dense_f64', '_dense_train', '_dense_ln'] if cls is SparseCINConv else ['_dense_eval', '_dense_train', '_dense_ln']
    params = [SimpleNamespace(x=torch.zeros(2, 8)) for _ in range(3)]
    for start, unfused in ((0, None), (1, None), (0, 1), (1, 2), (2, None)):
        plans = _plans(nb, start=start)
        if unfused is not None:
            plans[unfused] = None
        outs = [torch.zeros(2, 8) for p in plans if p is not None for _ in range(nb)]
        conv = _conv(cls, **kw)
        log = _stub(conv, plans, outs, {name: None for name in order})
        got = conv(*params, start_to_process=start)
        assert log[:len(order)] == [(name, start) for name in order]
        want, calls, k = [], [], 0
        for d in range(3):
            if d < start:
                want.append(params[d].x)
            elif d == unfused:
                want.append(('unfused', d))
                calls.append(('unfused', d, params[d]))
            else:
                want.append(('finished', d))
                calls.append(('finish', d, tuple(outs[k:k + nb])))
                k += nb
        assert len(got) == 3 and all(g is w or g == w for g, w in zip(got, want))
        assert all(got[d] is params[d].x for d in range(start))
        rest = log[len(order):]
        assert len(rest) == len(calls)
        for (kind, d, arg), (wkind, wd, warg) in zip(rest, calls):
            assert (kind, d) == (wkind, wd)
            if kind == 'finish':
                assert len(arg) == nb and all(a is w for a, w in zip(arg, warg))          # 2 / 3 / 4 tensors, these ones
            else:
                assert arg is warg


def test_plan_reports_its_shape_and_drops_out_with_a_combine_stage_only():
    lin = torch.nn.Linear(8, 8)
    stage = dense_train.Stage(lin, torch.nn.Identity())
    for nd, nb, depth in ((3, 2, 2), (2, 3, 2), (1, 4, 1), (2, 2, 3)):
        chains = [[[stage] * depth for _ in range(nb)] for _ in range(nd)]
        cb = [stage] * nd
        plan = dense_train._Plan(chains, cb, 0.25)
        assert (plan.nd, plan.nb, plan.depth) == (nd, nb, depth) and plan.out_drop == 0.25
        assert plan.chains is chains and plan.cb is cb
        assert len(list(plan.stages())) == nd * (nb * depth + 1)
        bare = dense_train._Plan(chains, None, 0.25)
        assert (bare.nd, bare.nb, bare.depth) == (nd, nb, depth) and bare.out_drop == 0.0 and bare.cb is None
        assert len(list(bare.stages())) == nd * nb * depth
        assert dense_train._Plan(chains, cb).out_drop == 0.0
