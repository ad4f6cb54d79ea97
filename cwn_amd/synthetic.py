"""Synthetic ring-lifted molecular complexes (no dataset is available offline).

`zinc_like_complexes` draws ZINC-shaped molecules (18-30 atoms, mean ~23; a tree backbone with 1-4
rings of size 5/6, fused pairs with probability 0.3; atom type in [0,28), bond type in [0,4),
data/datasets/zinc.py:29-30) and lifts each to a 2-complex with the ring lift restated from the
reference (data/utils.py:400-498: vertices, edges in lexicographic (u<v) order, induced cycles of
length <= max_ring as 2-cells; adjacency construction as build_adj, :103-138; boundary_index as
generate_cochain, :177-221).  Ring ids are canonical here (sorted by sorted vertex tuple); the
reference leaves them in Python-set order (:300-330).

Host-side numpy; it produces the INPUT of the hot path and is not on it.
"""
import itertools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .complex import Cochain, Complex, ComplexBatch


# ------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------
def random_molecule(rng: np.random.Generator, n_lo: int = 18, n_hi: int = 30,
                    ring_probs=(0.2, 0.4, 0.3, 0.1)) -> Tuple[int, List[Tuple[int, int]]]:
    """A connected molecule-like graph: (num_atoms, sorted list of bonds (u < v))."""
    target = int(rng.integers(n_lo, n_hi + 1))
    n_rings = int(rng.choice(len(ring_probs), p=ring_probs)) + 1
    deg: List[int] = []
    bonds = set()
    ring_bonds: List[Tuple[int, int]] = []      # bonds that belong to exactly one ring so far

    def new_atom() -> int:
        deg.append(0)
        return len(deg) - 1

    def bond(u: int, v: int):
        bonds.add((min(u, v), max(u, v)))
        deg[u] += 1
        deg[v] += 1

    def add_cycle(path: List[int]):
        for a, b in zip(path, path[1:] + path[:1]):
            if (min(a, b), max(a, b)) not in bonds:
                bond(a, b)
                ring_bonds.append((min(a, b), max(a, b)))

    for r in range(n_rings):
        k = 5 if rng.random() < 0.3 else 6
        fusable = [b for b in ring_bonds if deg[b[0]] <= 3 and deg[b[1]] <= 3]
        if r > 0 and fusable and rng.random() < 0.3:
            u, v = fusable[int(rng.integers(len(fusable)))]
            ring_bonds.remove((u, v))
            add_cycle([u] + [new_atom() for _ in range(k - 2)] + [v])
        else:
            cyc = [new_atom() for _ in range(k)]
            add_cycle(cyc)
            if r > 0:      # link the new ring to the molecule through 0-2 chain atoms
                free = [a for a in range(cyc[0]) if deg[a] < 4]
                prev = free[int(rng.integers(len(free)))]
                for _ in range(int(rng.integers(0, 3))):
                    a = new_atom()
                    bond(prev, a)
                    prev = a
                bond(prev, cyc[0])
    while len(deg) < target:
        free = [a for a in range(len(deg)) if deg[a] < 4]
        # prefer chain ends so side chains look like chains, not stars
        w = np.array([2.0 if deg[a] == 1 else 1.0 for a in free])
        prev = free[int(rng.choice(len(free), p=w / w.sum()))]
        bond(prev, new_atom())
    return len(deg), sorted(bonds)


def induced_cycles(n: int, bonds: Sequence[Tuple[int, int]], max_k: int) -> List[Tuple[int, ...]]:
    """All chordless cycles with 3..max_k vertices, each as a vertex tuple in cyclic order starting
    at its smallest vertex, sorted canonically (what graph-tool's induced subgraph isomorphism
    finds in data/utils.py:300-330; cross-checked against a networkx enumerator by the reference,
    data/helper_test.py:68-99)."""
    adj = [set() for _ in range(n)]
    for u, v in bonds:
        adj[u].add(v)
        adj[v].add(u)
    found = {}

    def extend(path: List[int]):
        s, last = path[0], path[-1]
        for w in adj[last]:
            if w == s:
                continue
            if w < s or w in path:
                continue
            # chordless: w may touch the path only at `last` (and at s when it closes the cycle)
            touches = adj[w].intersection(path)
            closing = s in touches
            if touches - {last, s}:
                continue
            if closing and len(path) + 1 >= 3:
                cyc = path + [w]
                key = tuple(sorted(cyc))
                if key not in found:
                    found[key] = tuple(cyc) if cyc[1] < cyc[-1] else tuple([cyc[0]] + cyc[:0:-1])
                continue   # a vertex adjacent to s cannot be an interior vertex of a longer cycle
            if len(path) + 1 < max_k:
                extend(path + [w])

    for s in range(n):
        for w in adj[s]:
            if w > s:
                extend([s, w])
    return [found[k] for k in sorted(found)]


def rook_4x4() -> Tuple[int, List[Tuple[int, int]]]:
    """The 4 x 4 rook's graph, one of the two strongly regular graphs SR(16, 6, 2, 2): vertices (i, j), adjacent when they
    share a row or a column.  (num_vertices, sorted list of edges (u < v))."""
    cells = [(i, j) for i in range(4) for j in range(4)]
    return 16, sorted((a, b) for a in range(16) for b in range(a + 1, 16)
                      if cells[a][0] == cells[b][0] or cells[a][1] == cells[b][1])


def shrikhande() -> Tuple[int, List[Tuple[int, int]]]:
    """The Shrikhande graph, the other SR(16, 6, 2, 2): vertices in Z4 x Z4, adjacent when their difference is +-(1, 0),
    +-(0, 1) or +-(1, 1).  1-WL (and 3-WL) cannot tell it from the rook's graph; the ring lift can."""
    cells = [(i, j) for i in range(4) for j in range(4)]
    steps = {(1, 0), (3, 0), (0, 1), (0, 3), (1, 1), (3, 3)}
    return 16, sorted((a, b) for a in range(16) for b in range(a + 1, 16)
                      if ((cells[a][0] - cells[b][0]) % 4, (cells[a][1] - cells[b][1]) % 4) in steps)


def relabel(n: int, bonds: Sequence[Tuple[int, int]], perm: Sequence[int]) -> Tuple[int, List[Tuple[int, int]]]:
    """The same graph with vertex v renamed perm[v]: an isomorphic copy."""
    return n, sorted((min(int(perm[u]), int(perm[v])), max(int(perm[u]), int(perm[v]))) for u, v in bonds)


def sr_lift(n: int, bonds: Sequence[Tuple[int, int]], max_k: int = 6, dtype=torch.float64) -> Complex:
    """The ring lift of a featureless graph as the strongly-regular-graph experiments feed it: constant vertex features,
    every higher cell the sum of its vertices' (edges 2, a k-ring k), in `dtype`."""
    cx = ring_lift(n, bonds, torch.ones(n, 1, dtype=dtype), torch.full((len(bonds), 1), 2.0, dtype=dtype), max_k=max_k)
    if cx.dimension >= 2:
        sizes = torch.bincount(cx.cochains[2].boundary_index[1]).to(dtype).unsqueeze(1)
        cx.cochains[2].x = sizes
    return cx


# ------------------------------------------------------------------------------------------------
# ring lift
# ------------------------------------------------------------------------------------------------
def ring_lift(n: int, bonds: Sequence[Tuple[int, int]], vx: torch.Tensor,
              ex: Optional[torch.Tensor] = None, max_k: int = 6, include_down_adj: bool = False,
              y: Optional[torch.Tensor] = None, rx: Optional[torch.Tensor] = None) -> Complex:
    """compute_ring_2complex (data/utils.py:400-498) restated: returns a cwn_amd Complex."""
    bonds = sorted((min(u, v), max(u, v)) for u, v in bonds)
    edge_id = {b: i for i, b in enumerate(bonds)}
    rings = induced_cycles(n, bonds, max_k)
    ring_edges = []
    for ring in rings:
        es = sorted(tuple(sorted((ring[i], ring[(i + 1) % len(ring)]))) for i in range(len(ring)))
        ring_edges.append([edge_id[e] for e in es])          # get_ring_boundaries (:355-367)

    def pairs(groups):
        idx, shared = [], []
        for gid, members in enumerate(groups):
            for a, b in itertools.combinations(members, 2):
                idx += [(a, b), (b, a)]
                shared += [gid, gid]
        return idx, shared

    def lower(members_of_cell, n_lower):
        """cells sharing a boundary cell: for each lower cell, all pairs of its cofaces."""
        cof = [[] for _ in range(n_lower)]
        for cid, members in enumerate(members_of_cell):
            for m in members:
                cof[m].append(cid)
        return pairs(cof)

    def idx_tensor(lst):
        return torch.tensor(lst, dtype=torch.long).t().contiguous() if lst else None

    def vec_tensor(lst):
        return torch.tensor(lst, dtype=torch.long) if lst else None

    dim = 2 if rings else (1 if bonds else 0)
    v_up, v_cob = pairs([list(b) for b in bonds])
    cochains = [Cochain(dim=0, x=vx, upper_index=idx_tensor(v_up), shared_coboundaries=vec_tensor(v_cob),
                        num_cells_up=len(bonds) if dim >= 1 else 0, num_cells=n)]
    if dim >= 1:
        e_up, e_cob = pairs(ring_edges)
        e_down, e_bnd = lower([list(b) for b in bonds], n) if include_down_adj else ([], [])
        b_index = torch.tensor([[v for b in bonds for v in b],
                                [i for i in range(len(bonds)) for _ in range(2)]], dtype=torch.long)
        cochains.append(Cochain(dim=1, x=ex, upper_index=idx_tensor(e_up),
                                shared_coboundaries=vec_tensor(e_cob), lower_index=idx_tensor(e_down),
                                shared_boundaries=vec_tensor(e_bnd), boundary_index=b_index,
                                num_cells=len(bonds), num_cells_down=n,
                                num_cells_up=len(rings) if dim >= 2 else 0))
    if dim >= 2:
        r_down, r_bnd = lower(ring_edges, len(bonds)) if include_down_adj else ([], [])
        b_index = torch.tensor([[e for es in ring_edges for e in es],
                                [i for i, es in enumerate(ring_edges) for _ in es]], dtype=torch.long)
        cochains.append(Cochain(dim=2, x=rx, lower_index=idx_tensor(r_down),
                                shared_boundaries=vec_tensor(r_bnd), boundary_index=b_index,
                                num_cells=len(rings), num_cells_down=len(bonds), num_cells_up=0))
    return Complex(*cochains, y=y, dimension=dim)


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def zinc_like_complexes(num: int, seed: int = 0, max_ring: int = 6, n_lo: int = 18, n_hi: int = 30,
                        atom_types: int = 28, bond_types: int = 4,
                        include_down_adj: bool = False, size_dist: str = 'uniform') -> List[Complex]:
    """`num` ZINC-shaped ring-lifted complexes with integer atom / bond types as [N,1] floats
    (the form EmbedSparseCIN expects, mp/molec_models.py:95-99).  size_dist: 'uniform' on [n_lo, n_hi] (SURVEY.md 8d's
    generator: 18 - 30), or 'zinc': the published size statistics of the ZINC-12k subset the reference trains on (9 - 37 heavy
    atoms, mean 23.2, standard deviation ~4.6: a clipped normal -- about 2 % of the molecules have more than 32 atoms (what a workgroup of the layer kernel held at width 128 until round 4), the
    most one workgroup of the 16-wave layer kernel holds at width 128)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        if size_dist == 'zinc':
            k = int(np.clip(np.rint(rng.normal(23.2, 4.6)), 9, 37))
            n, bonds = random_molecule(rng, k, k)
        else:
            n, bonds = random_molecule(rng, n_lo, n_hi)
        vx = torch.from_numpy(rng.integers(0, atom_types, size=(n, 1))).float()
        ex = torch.from_numpy(rng.integers(0, bond_types, size=(len(bonds), 1))).float()
        y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
        out.append(ring_lift(n, bonds, vx, ex, max_k=max_ring, include_down_adj=include_down_adj, y=y))
    return out


def zinc_like_batch(batch_size: int = 128, seed: int = 0, max_ring: int = 6, device=None,
                    **kw) -> ComplexBatch:
    b = ComplexBatch.from_complex_list(zinc_like_complexes(batch_size, seed, max_ring, **kw), max_dim=2)
    return b.to(device) if device is not None else b


def batch_stats(batch: ComplexBatch) -> dict:
    """Cell and adjacency-entry counts (the N_d, E_up, B of SURVEY.md §8)."""
    s = {}
    for d in range(batch.dimension + 1):
        c = batch.cochains[d]
        s[f'N{d}'] = int(c.num_cells)
        s[f'E_up{d}'] = int(c.upper_index.size(1)) if c.upper_index is not None else 0
        s[f'E_down{d}'] = int(c.lower_index.size(1)) if c.lower_index is not None else 0
        s[f'B{d}'] = int(c.boundary_index.size(1)) if c.boundary_index is not None else 0
    s['cells'] = sum(s[f'N{d}'] for d in range(batch.dimension + 1))
    return s


# ------------------------------------------------------------------------------------------------
# molhiv-like (BASELINE config 3) and REDDIT-like clique complexes (config 5)
# ------------------------------------------------------------------------------------------------
def molhiv_like_complexes(num: int, seed: int = 0, max_ring: int = 6, n_lo: int = 10, n_hi: int = 60,
                          atom_dims=(119, 4, 12, 12, 10, 6, 6, 2, 2), bond_dims=(5, 6, 2), tail: float = 0.0,
                          tail_lo: int = 120, tail_hi: int = 220) -> List[Complex]:
    """ogbg-molhiv-shaped inputs: 10-60 atoms, 9 integer atom-feature columns, 3 integer bond-feature
    columns (OGB convention), ring lift with max_ring.  `tail`: the probability of a molecule from the dataset's heavy tail
    instead -- ogbg-molhiv's published statistics (41 127 molecules, 25.5 atoms on average, the largest 222) put a few
    molecules of 120 - 220 atoms in every 10 000: complexes beyond what one workgroup of the blocked layer kernel holds, which
    the generator of SURVEY.md 8d (10 - 60 atoms) never produces (`molhiv_real_tail`, tail = 5e-4)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        lo_, hi_ = (tail_lo, tail_hi) if (tail > 0.0 and rng.random() < tail) else (n_lo, n_hi)
        n, bonds = random_molecule(rng, lo_, hi_, ring_probs=(0.25, 0.35, 0.25, 0.15))
        vx = torch.from_numpy(np.stack([rng.integers(0, d, size=n) for d in atom_dims], 1))
        ex = torch.from_numpy(np.stack([rng.integers(0, d, size=len(bonds)) for d in bond_dims], 1))
        y = torch.from_numpy(rng.integers(0, 2, size=(1, 1)).astype(np.float32))
        out.append(ring_lift(n, bonds, vx, ex, max_k=max_ring, y=y))
    return out


def preferential_attachment_graph(rng: np.random.Generator, n: int, m: int = 2, hubs: int = 2,
                                  hub_degree: int = 100) -> List[Tuple[int, int]]:
    """A REDDIT-like discussion graph: preferential attachment (each new vertex links to `m`
    earlier ones, probability ~ degree) with `hubs` vertices forced to degree >= hub_degree."""
    edges = set()
    targets = [0, 1]
    edges.add((0, 1))
    for v in range(2, n):
        picks = set()
        while len(picks) < min(m, v):
            picks.add(int(targets[int(rng.integers(len(targets)))]))
        for u in picks:
            edges.add((min(u, v), max(u, v)))
            targets += [u, v]
    deg = np.zeros(n, dtype=np.int64)
    for u, v in edges:
        deg[u] += 1
        deg[v] += 1
    for h in np.argsort(-deg)[:hubs]:
        need = hub_degree - int(deg[h])
        if need > 0:
            others = [int(v) for v in rng.permutation(n) if v != h and (min(h, v), max(h, v)) not in edges]
            for v in others[:need]:
                edges.add((min(int(h), v), max(int(h), v)))
    return sorted(edges)


def clique_lift(n: int, edges: Sequence[Tuple[int, int]], vx: torch.Tensor, max_dim: int = 2,
                init_method: str = 'sum', y: Optional[torch.Tensor] = None,
                include_down_adj: bool = False) -> Complex:
    """compute_clique_complex_with_gudhi (data/utils.py:224-272) restated for expansion_dim <= 2:
    vertices, edges in lexicographic (u<v) order, triangles in lexicographic order (the order of a
    gudhi SimplexTree traversal); upper adjacencies as build_adj (:103-138); boundaries of a
    simplex in itertools.combinations order (:40-42); features of higher cells = reduce of their
    vertices' features (construct_features, :141-156)."""
    edges = sorted((min(u, v), max(u, v)) for u, v in edges)
    edge_id = {e: i for i, e in enumerate(edges)}
    nbrs = [set() for _ in range(n)]
    for u, v in edges:
        nbrs[u].add(v)
        nbrs[v].add(u)
    tris = []
    if max_dim >= 2:
        for u, v in edges:
            for w in sorted(nbrs[u] & nbrs[v]):
                if w > v:
                    tris.append((u, v, w))
        tris.sort()
    tri_edges = [[edge_id[(a, b)], edge_id[(a, c)], edge_id[(b, c)]] for a, b, c in tris]

    def pairs(groups):
        idx, shared = [], []
        for gid, members in enumerate(groups):
            for a, b in itertools.combinations(members, 2):
                idx += [(a, b), (b, a)]
                shared += [gid, gid]
        return idx, shared

    def idx_tensor(lst):
        return torch.tensor(lst, dtype=torch.long).t().contiguous() if lst else None

    def vec_tensor(lst):
        return torch.tensor(lst, dtype=torch.long) if lst else None

    def reduce_feats(groups):
        if not groups:
            return None
        g = torch.tensor(groups, dtype=torch.long)
        f = vx[g]                                    # [cells, k, F]
        return f.sum(1) if init_method in ('sum', 'add') else f.mean(1)

    def lower(members_of_cell, n_lower):
        cof = [[] for _ in range(n_lower)]
        for cid, members in enumerate(members_of_cell):
            for m in members:
                cof[m].append(cid)
        return pairs(cof)

    dim = 2 if tris else (1 if edges else 0)
    v_up, v_cob = pairs([list(e) for e in edges])
    cochains = [Cochain(dim=0, x=vx, upper_index=idx_tensor(v_up), shared_coboundaries=vec_tensor(v_cob),
                        num_cells=n, num_cells_up=len(edges) if dim >= 1 else 0)]
    if dim >= 1:
        e_up, e_cob = pairs(tri_edges)
        e_down, e_bnd = lower([list(e) for e in edges], n) if include_down_adj else ([], [])
        b_index = torch.tensor([[v for e in edges for v in e],
                                [i for i in range(len(edges)) for _ in range(2)]], dtype=torch.long)
        cochains.append(Cochain(dim=1, x=reduce_feats([list(e) for e in edges]), upper_index=idx_tensor(e_up),
                                shared_coboundaries=vec_tensor(e_cob), lower_index=idx_tensor(e_down),
                                shared_boundaries=vec_tensor(e_bnd), boundary_index=b_index,
                                num_cells=len(edges), num_cells_down=n,
                                num_cells_up=len(tris) if dim >= 2 else 0))
    if dim >= 2:
        t_down, t_bnd = lower(tri_edges, len(edges)) if include_down_adj else ([], [])
        b_index = torch.tensor([[e for es in tri_edges for e in es],
                                [i for i in range(len(tris)) for _ in range(3)]], dtype=torch.long)
        cochains.append(Cochain(dim=2, x=reduce_feats([list(t) for t in tris]), lower_index=idx_tensor(t_down),
                                shared_boundaries=vec_tensor(t_bnd), boundary_index=b_index,
                                num_cells=len(tris), num_cells_down=len(edges), num_cells_up=0))
    return Complex(*cochains, y=y, dimension=dim)


def reddit_like_complexes(num: int = 32, seed: int = 0, n_lo: int = 200, n_hi: int = 1000,
                          init_method: str = 'mean') -> List[Complex]:
    """REDDIT-BINARY-shaped inputs (exp/scripts/mpsn-redditb.sh): large irregular graphs with 1-3
    hubs of degree >= 100, a constant scalar vertex feature, clique lift to dimension 2,
    higher-cell features by `init_method` (mean -> all ones)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        n = int(rng.integers(n_lo, n_hi + 1))
        edges = preferential_attachment_graph(rng, n, m=int(rng.integers(1, 4)), hubs=int(rng.integers(1, 4)),
                                              hub_degree=int(rng.integers(100, 200)))
        vx = torch.ones(n, 1)
        y = torch.from_numpy(rng.integers(0, 2, size=1))
        out.append(clique_lift(n, edges, vx, max_dim=2, init_method=init_method, y=y))
    return out


# ------------------------------------------------------------------------------------------------
# CSL: circulant skip-link graphs (the reference's CSL dataset, exp/scripts/cwn-csl.sh)
# ------------------------------------------------------------------------------------------------
CSL_NODES = 41
CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)        # one isomorphism class per skip length: ten classes


def csl_graph(skip: int, n: int = CSL_NODES) -> Tuple[int, List[Tuple[int, int]]]:
    """C_{n, skip}: the cycle 0 - 1 - ... - (n - 1) - 0 plus a link from every vertex to the one `skip` further.  Regular of
    degree 4, so 1-WL sees one graph in all of them; the rings tell them apart.  (num_vertices, sorted edges (u < v))."""
    edges = set()
    for v in range(n):
        for w in ((v + 1) % n, (v + skip) % n):
            edges.add((min(v, w), max(v, w)))
    return n, sorted(edges)


def csl_graphs(num: int = 150, seed: int = 0, max_ring: int = 8) -> List[Complex]:
    """`num` ring-lifted CSL complexes: graph k is a randomly relabelled copy of C_{41, CSL_SKIPS[k % 10]} with the class
    k % 10 as its target (int64), featureless as the reference feeds them (data/datasets/csl.py: atom type 0 on every
    vertex, bond type 0 on every edge -- [N, 1] floats, the form EmbedSparseCIN expects).  max_ring 8 is cwn-csl.sh's."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(num):
        cls = k % len(CSL_SKIPS)
        n, edges = csl_graph(CSL_SKIPS[cls])
        n, edges = relabel(n, edges, rng.permutation(n))
        out.append(ring_lift(n, edges, torch.zeros(n, 1), torch.zeros(len(edges), 1), max_k=max_ring,
                             y=torch.tensor([cls], dtype=torch.long)))
    return out


# ------------------------------------------------------------------------------------------------
# edge flows on a triangulated grid (the FLOW experiments of the reference)
# ------------------------------------------------------------------------------------------------
_HOLES = ((0.2, 0.2, 0.4, 0.4), (0.6, 0.6, 0.8, 0.8))          # (x0, y0, x1, y1), closed rectangles
_START, _END = (0.0, 0.8, 0.2, 1.0), (0.8, 0.0, 1.0, 0.2)      # the two opposite corner regions of a path
_CHECKPOINTS = ((0.0, 0.0, 0.2, 0.2), (0.8, 0.8, 1.0, 1.0))    # class 0 passes below the first hole, class 1 above the second


def _in_rect(points: np.ndarray, rect) -> np.ndarray:
    x0, y0, x1, y1 = rect
    t = 1e-9
    return (points[:, 0] >= x0 - t) & (points[:, 0] <= x1 + t) & (points[:, 1] >= y0 - t) & (points[:, 1] <= y1 + t)


def adjacency_from_boundary(B: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(index [2, P] int64, orient [P] float32) of the columns of B that meet: the off-diagonal entries of B^T B (each +-1 for
    a simplicial complex).  Pair (i, j), j < i, is stored as the two consecutive entries i -> j, j -> i with ONE sign, pairs
    in row-major order of (i, j) -- the layout of data/datasets/flow_utils.py:199-230."""
    A = np.rint(B.T.astype(np.float32) @ B.astype(np.float32)).astype(np.int64)      # (small integers: exact in fp32)
    ii, jj = np.nonzero(np.tril(A, -1))
    v = A[ii, jj]
    assert np.all(np.abs(v) == 1), 'columns that share more than one row: not a simplicial complex'
    index = np.empty((2, 2 * ii.size), dtype=np.int64)
    index[0, 0::2], index[1, 0::2] = ii, jj
    index[0, 1::2], index[1, 1::2] = jj, ii
    return index, np.repeat(v, 2).astype(np.float32)


def edge_flow_mesh(side: int, holes: bool = True) -> dict:
    """A `side` x `side` grid of points on the unit square, every grid cell cut into two triangles, without the triangles
    whose centroid lies in one of the two rectangular holes (`holes`).  Returns the points [V, 2], the edges [E, 2] (u < v,
    lexicographic), the triangles [T, 3] (sorted vertices), the boundary matrices B1 [V, E] and B2 [E, T] in the
    orientation "from the smaller to the larger vertex" (B1 B2 = 0), and the lower / upper adjacency of the edges with
    their relative orientations (`adjacency_from_boundary` of B1 and of B2^T)."""
    if side < 2:
        raise ValueError('edge_flow_mesh needs side >= 2')
    g = np.arange(side) / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    vid = lambda i, j: i * side + j
    tris = []
    for i in range(side - 1):
        for j in range(side - 1):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
            tris += [(a, b, d), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, c), (b, c, d)]
    tris = np.array(tris, dtype=np.int64)
    if holes:                                                    # a triangle belongs to a hole when its centroid does
        mid = pts[tris].mean(1)
        tris = tris[~(_in_rect(mid, _HOLES[0]) | _in_rect(mid, _HOLES[1]))]
    if len(tris) == 0:
        raise ValueError(f'side={side}: the holes leave no triangle')
    used = np.unique(tris)                                       # vertices that lost every triangle go too
    renum = np.full(side * side, -1, dtype=np.int64)
    renum[used] = np.arange(used.size)
    pts, tris = pts[used], np.sort(renum[tris], 1)
    edges = np.unique(np.concatenate([tris[:, [0, 1]], tris[:, [0, 2]], tris[:, [1, 2]]]), axis=0)
    V, E, T = len(pts), len(edges), len(tris)
    eid = {(int(u), int(v)): k for k, (u, v) in enumerate(edges)}
    B1 = np.zeros((V, E), dtype=np.int8)
    B1[edges[:, 0], np.arange(E)] = -1
    B1[edges[:, 1], np.arange(E)] = 1
    B2 = np.zeros((E, T), dtype=np.int8)
    for t, (a, b, c) in enumerate(tris):                         # boundary of [a, b, c], a < b < c: [b, c] - [a, c] + [a, b]
        B2[eid[(int(b), int(c))], t] = 1
        B2[eid[(int(a), int(c))], t] = -1
        B2[eid[(int(a), int(b))], t] = 1
    lower_index, lower_orient = adjacency_from_boundary(B1)
    upper_index, upper_orient = adjacency_from_boundary(B2.T)
    nbrs = [[] for _ in range(V)]
    for u, v in edges:
        nbrs[int(u)].append(int(v))
        nbrs[int(v)].append(int(u))
    return dict(points=pts, edges=edges, triangles=tris, B1=B1, B2=B2, edge_id=eid, neighbours=nbrs,
                lower_index=lower_index, lower_orient=lower_orient, upper_index=upper_index, upper_orient=upper_orient)


def _flow_path(mesh: dict, cls: int, rng: np.random.Generator) -> List[int]:
    """A vertex path from the start corner through the class's checkpoint region to the end corner: greedy towards the
    current target over unvisited neighbours, one step in ten random (data/datasets/flow_utils.py:142-196, restated)."""
    pts, nbrs = mesh['points'], mesh['neighbours']
    pick = lambda rect: int(rng.choice(np.nonzero(_in_rect(pts, rect))[0]))
    for _ in range(1000):
        start, end, ckpt = pick(_START), pick(_END), pick(_CHECKPOINTS[cls])
        path, seen, v, reached = [start], set(), start, False
        while v != end:
            seen.add(v)
            reached = reached or v == ckpt
            cand = [u for u in nbrs[v] if u not in seen]
            if not cand:
                break                                            # walked into a dead end: draw another path
            if rng.random() < 0.1:
                v = cand[int(rng.integers(len(cand)))]
            else:
                d = ((pts[cand] - pts[end if reached else ckpt]) ** 2).sum(1)
                v = cand[int(np.argmin(d))]
            path.append(v)
        if v == end:
            return path
    raise RuntimeError('no path found: the mesh is too coarse for the corner regions')


def edge_flows(n_complexes: int, side: int, seed: int, holes: bool = True, flip=None) -> List[Cochain]:
    """`n_complexes` edge-flow cochains on one `edge_flow_mesh(side, holes)`: the FLOW task of the reference
    (data/datasets/flow_utils.py:93-252) restated.  x [E, 1] is +-1 on the edges of a path from one corner region of the
    square to the opposite one (the sign: along or against the edge's orientation) and 0 elsewhere; y says around which
    of the two holes the path went (the first half of the list is class 0).  Every cochain gets its own random change of
    edge orientations T = diag(t), t in {+-1}^E: B1 -> B1 T, B2 -> T B2, x -> T x, hence for the adjacencies
    orient_ij -> t_i t_j orient_ij -- which is how it is applied here, once per cochain, to the mesh's adjacency.
    `flip`: an explicit t ([E] of +-1) for every cochain instead (the draws of the paths do not depend on it).
    Deterministic per (n_complexes, side, seed, holes)."""
    mesh = edge_flow_mesh(side, holes)
    E = len(mesh['edges'])
    rng_path, rng_flip = np.random.default_rng([int(seed), 0]), np.random.default_rng([int(seed), 1])
    lo, up = mesh['lower_index'], mesh['upper_index']
    lower_index, upper_index = torch.from_numpy(lo), torch.from_numpy(up)
    out = []
    for k in range(n_complexes):
        cls = 0 if k < n_complexes // 2 or n_complexes == 1 else 1
        path = _flow_path(mesh, cls, rng_path)
        x = np.zeros((E, 1), dtype=np.float32)
        for a, b in zip(path[:-1], path[1:]):
            x[mesh['edge_id'][(min(a, b), max(a, b))], 0] = 1.0 if a < b else -1.0
        t = rng_flip.integers(0, 2, size=E) * 2 - 1 if flip is None else np.asarray(flip).reshape(E)
        t = t.astype(np.float32)
        out.append(Cochain(dim=1, x=torch.from_numpy(x * t[:, None]),
                           lower_index=lower_index.clone(), upper_index=upper_index.clone(),
                           lower_orient=torch.from_numpy(mesh['lower_orient'] * t[lo[0]] * t[lo[1]]),
                           upper_orient=torch.from_numpy(mesh['upper_orient'] * t[up[0]] * t[up[1]]),
                           y=torch.tensor([cls])))
    return out


# ------------------------------------------------------------------------------------------------
# ring transfer (data/datasets/ring_utils.py:61-103, data/datasets/ringtransfer.py:60-76)
# ------------------------------------------------------------------------------------------------
def ring_transfer(nodes: int, samples: int, classes: int = 5) -> List[Complex]:
    """The RING-TRANSFER dataset restated: `samples` rings of `nodes` vertices, lifted with max_k = nodes (one two-cell with
    all `nodes` edges on its boundary).  Vertex features are constant one, zero at vertex 0 (the target) and the one-hot
    label at vertex nodes // 2 (the source, on the other side of the ring); complex i carries label i // (samples //
    classes); edge and two-cell features are zeroed; `nodes.mask` marks vertex 0.  Three cellular layers carry the label
    across for every ring size (the two-cell touches every edge), a GIN needs nodes / 2.  The complexes of one call share
    their index tensors (they all are the same ring)."""
    if nodes < 3 or classes < 1 or samples < classes or samples % classes != 0:
        raise ValueError('a ring has at least 3 vertices, and `samples` is a positive multiple of `classes`')
    per_class = samples // classes
    bonds = [(i, i + 1) for i in range(nodes - 1)] + [(0, nodes - 1)]
    zeros = torch.zeros(nodes, classes)
    shape = ring_lift(nodes, bonds, zeros, zeros.clone(), max_k=nodes, rx=torch.zeros(1, classes))
    assert shape.dimension == 2 and shape.two_cells.num_cells == 1
    v, e, r = shape.nodes, shape.edges, shape.two_cells
    mask = torch.zeros(nodes, dtype=torch.bool)
    mask[0] = True
    xs = []
    for label in range(classes):
        x = torch.ones(nodes, classes)
        x[0, :] = 0.0
        x[nodes // 2, :] = 0.0
        x[nodes // 2, label] = 1.0
        xs.append(x)
    out = []
    for i in range(samples):
        label = i // per_class
        out.append(Complex(
            Cochain(dim=0, x=xs[label], upper_index=v.upper_index, shared_coboundaries=v.shared_coboundaries,
                    num_cells_up=nodes, num_cells=nodes, mask=mask),
            Cochain(dim=1, x=e.x, upper_index=e.upper_index, shared_coboundaries=e.shared_coboundaries,
                    boundary_index=e.boundary_index, num_cells=nodes, num_cells_down=nodes, num_cells_up=1),
            Cochain(dim=2, x=r.x, boundary_index=r.boundary_index, num_cells=1, num_cells_down=nodes, num_cells_up=0),
            y=torch.tensor([label], dtype=torch.long), dimension=2))
    return out
