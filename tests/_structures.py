"""Small complexes the molecular generators do not produce, built through cwn_amd.lifting: triangulated strips, complete
graphs, single rings, stars, paths and bags of tiny complexes (isolated vertices and lone bonds among them).  Every
builder returns a list of Complex with zero features of width 1; the tests collate them and fill in their own values.
`duplicate_entries` repeats upper-adjacency entries inside their complex's slice (summed with multiplicity)."""
import numpy as np
import torch


def _z(n):
    return torch.zeros(n, 1)


def _clique(n, edges):
    from cwn_amd import lifting
    return lifting.clique_lift(n, sorted(edges), _z(n), max_dim=2, y=torch.zeros(1))


def _ring(n, bonds, max_k=18):
    from cwn_amd import lifting
    bonds = sorted((min(u, v), max(u, v)) for u, v in bonds)
    return lifting.ring_lift(n, bonds, _z(n), _z(len(bonds)), max_k=max_k, y=torch.zeros(1))


def strip(t):
    """Triangulated strip of t triangles: vertices 0 .. t + 1, edges (i, i + 1) and (i, i + 2); 2 t + 1 edges."""
    n = t + 2
    return [_clique(n, [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)])]


def clique(n):
    """K_n: n (n - 1) / 2 edges, n (n - 1) (n - 2) / 6 triangles."""
    return [_clique(n, [(i, j) for i in range(n) for j in range(i + 1, n)])]


def ring(k):
    """One cycle of k vertices: a single 2-cell with k boundary edges, k (k - 1) upper-adjacency entries among them."""
    return [_ring(k, [(i, (i + 1) % k) for i in range(k)])]


def star(k):
    """A hub (vertex 0) with k leaves: the hub is the source of k upper-adjacency entries."""
    return [_ring(k + 1, [(0, i) for i in range(1, k + 1)])]


def path(n):
    """n vertices in a line, n - 1 edges, no 2-cell."""
    return [_ring(n, [(i, i + 1) for i in range(n - 1)])]


def vertex():
    return [_ring(1, [])]


def bond():
    return [_ring(2, [(0, 1)])]


BAG_KINDS = ('vertex', 'bond', 'triangle', 'K4', 'ring5', 'path3')


def bag(C, seed):
    """C complexes drawn uniformly from BAG_KINDS: complexes that are empty in dimension 1 and / or 2 among full ones."""
    rng = np.random.default_rng(seed)
    make = {'vertex': vertex, 'bond': bond, 'triangle': lambda: clique(3), 'K4': lambda: clique(4),
            'ring5': lambda: ring(5), 'path3': lambda: path(3)}
    return [make[BAG_KINDS[int(rng.integers(0, len(BAG_KINDS)))]]()[0] for _ in range(C)]


def mixed():
    """A lone bond (an edges item with no 2-cell: TOP rows absent), an isolated vertex (a record without entries) and a
    strip of two triangles."""
    return bond() + vertex() + strip(2)


# name -> (builder, max_dim of the batch, the owner form of the backward has a table at F = 128, at F = 64).  The last two
# are what tests/test_bwd_items.py asserts on the CPU; the GPU tests pick their cases by them.  (At F = 128 the limit that
# binds is usually the LDS budget of an item, not the row caps.)
CASES = {
    'K6': (lambda: clique(6), 2, True, True),
    'K7': (lambda: clique(7), 2, False, True),
    'strip16': (lambda: strip(16), 2, True, True),
    'strip17': (lambda: strip(17), 2, False, True),
    'strip33': (lambda: strip(33), 2, False, True),
    'ring18': (lambda: ring(18), 2, True, True),
    'ring16': (lambda: ring(16), 2, True, True),
    'star32': (lambda: star(32), 1, True, True),
    'star33': (lambda: star(33), 1, False, True),
    'star64': (lambda: star(64), 1, False, True),
    'star65': (lambda: star(65), 1, False, False),
    'path33': (lambda: path(33), 2, True, True),
    'path34': (lambda: path(34), 2, False, True),
    'mixed': (mixed, 2, True, True),
    'bag600': (lambda: bag(600, 0), 2, True, True),
}


def cases_with_table(F):
    return [k for k, v in CASES.items() if v[2 if F == 128 else 3]]


def host_batch(name):
    """The collated host batch of a case of CASES."""
    make, max_dim = CASES[name][:2]
    return collate(make(), max_dim)


def collate(complexes, max_dim):
    from cwn_amd.complex import ComplexBatch
    return ComplexBatch.from_complex_list(complexes, max_dim=max_dim)


def duplicate_entries(batch, rng):
    """Repeat a few entries of every upper adjacency (dimensions 0 and 1) of a collated host batch inside their complex's
    slice -- the entries stay grouped by complex, as the item tables require -- and update __slices__.  In place."""
    for d in range(2):
        c = batch.cochains.get(d)
        if c is None or d + 1 not in batch.cochains or c.upper_index is None or c.upper_index.size(1) == 0:
            continue
        sl = list(c.__slices__['upper_index'])
        cols, new_sl = [], [0]
        for s0, e0 in zip(sl[:-1], sl[1:]):
            idx = list(range(s0, e0))
            if idx and rng.random() < 0.5:
                idx += [int(rng.choice(idx))] * int(rng.integers(1, 3))
            cols += idx
            new_sl.append(len(cols))
        perm = torch.tensor(cols, dtype=torch.long)
        c.upper_index = c.upper_index[:, perm].contiguous()
        c.shared_coboundaries = c.shared_coboundaries[perm].contiguous()
        c.__slices__['upper_index'] = new_sl
        if 'shared_coboundaries' in c.__slices__:
            c.__slices__['shared_coboundaries'] = new_sl
    return batch
