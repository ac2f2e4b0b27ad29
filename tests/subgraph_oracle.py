"""numpy oracle of radargnn_amd.subgraph (csrc/subgraph.hip), restated rule by rule from include/rgnn.h:

    flags      a node is kept iff its mask entry is set; an edge is kept iff it is SOUND, its own mask entry is set and both its ends
               are kept.  Unsound, each with its status bit: an end outside [0, N); the source's graph outside [0, B); ends in two
               graphs; the source of the edge before it lying in a later graph
    ids        new_id = exclusive cumulative count of the node flags (-1 for a dropped node)
    offsets    ptr'[g] = kept nodes before ptr[g]; _edge_ptr'[g] = kept edges whose source lies in a graph before g
    gather     rows move with their node / edge, in order
    degree     |in U out| of the kept graph
and the edge-pair hash in uint64.  tests/test_subgraph_oracle.py checks all of it against plain Python loops."""
import numpy as np

BAD_ENDPOINT, CROSS_GRAPH, EDGE_ORDER, BAD_GRAPH = 8192, 16384, 32768, 65536
_M = np.uint64


def mix(z):
    """the 64-bit finaliser of rgnn.h on uint64 (arrays or scalars), arithmetic mod 2^64"""
    z = np.asarray(z).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + _M(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
        return z ^ (z >> _M(31))


def pair_draw(seed: int, s, t):
    """the 24-bit draw of the unordered pair {s, t}; seed: any Python int, taken mod 2^64"""
    s, t = np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64)
    lo, hi = np.minimum(s, t).astype(np.uint64), np.maximum(s, t).astype(np.uint64)
    key = (lo << _M(32)) | hi
    return (mix(mix(_M(seed % 2 ** 64)) ^ key) >> _M(40)).astype(np.int64)


def threshold(p: float) -> int:
    return int(np.floor(p * 2 ** 24))


def pair_mask(edge_index, n: int, seed: int, p: float):
    s, t = edge_index
    inside = (s >= 0) & (s < n) & (t >= 0) & (t < n)
    return inside & (pair_draw(seed, s, t) >= threshold(p))


def edge_flags(edge_index, batch, n_graphs, keep_nodes, keep_edges):
    """-> (kept bool [E], status): the rules in order, every index checked before it is one"""
    s, t = edge_index
    n, e = len(batch), edge_index.shape[1]
    kn = np.ones(n, bool) if keep_nodes is None else np.asarray(keep_nodes).astype(bool)
    ke = np.ones(e, bool) if keep_edges is None else np.asarray(keep_edges).astype(bool)
    inside = (s >= 0) & (s < n) & (t >= 0) & (t < n)
    sc, tc = np.where(inside, s, 0), np.where(inside, t, 0)
    gs, gt = batch[sc] if n else np.zeros(e, np.int64), batch[tc] if n else np.zeros(e, np.int64)
    graph_ok = inside & (gs >= 0) & (gs < n_graphs)
    same = graph_ok & (gs == gt)
    prev = np.concatenate(([-1], s[:-1])) if e else s
    prev_in = (prev >= 0) & (prev < n)
    g_prev = batch[np.where(prev_in, prev, 0)] if n else np.zeros(e, np.int64)
    ordered = same & ~(prev_in & (g_prev > gs))
    status = 0
    for bit, bad in ((BAD_ENDPOINT, ~inside), (BAD_GRAPH, inside & ~graph_ok), (CROSS_GRAPH, graph_ok & ~same), (EDGE_ORDER, same & ~ordered)):
        status |= bit if bad.any() else 0
    return ordered & ke & kn[sc] & kn[tc], status


def subgraph(edge_index, batch, ptr, keep_nodes=None, keep_edges=None, node_attrs=None, edge_attrs=None):
    """-> dict: edge_index, batch, ptr, edge_ptr, node_ids, edge_ids, new_id, status, node_attrs, edge_attrs"""
    edge_index, batch, ptr = np.asarray(edge_index, np.int64).reshape(2, -1), np.asarray(batch, np.int64), np.asarray(ptr, np.int64)
    n, b = len(batch), len(ptr) - 1
    kn = np.ones(n, bool) if keep_nodes is None else np.asarray(keep_nodes).astype(bool)
    kept_e, status = edge_flags(edge_index, batch, b, keep_nodes, keep_edges)
    before = np.concatenate(([0], np.cumsum(kn)))                         # kept nodes before i
    new_id = np.where(kn, before[:-1], -1).astype(np.int32)
    if ((ptr < 0) | (ptr > n)).any():
        status |= BAD_GRAPH
    node_ids, edge_ids = np.nonzero(kn)[0].astype(np.int64), np.nonzero(kept_e)[0].astype(np.int64)
    s, t = edge_index[:, edge_ids]
    graph_of_edge = batch[s]
    return {"edge_index": np.stack((new_id[s], new_id[t])).astype(np.int64).reshape(2, -1), "batch": batch[node_ids],
            "ptr": before[np.clip(ptr, 0, n)].astype(np.int64),
            "edge_ptr": np.array([(graph_of_edge < g).sum() for g in range(b + 1)], dtype=np.int64),
            "node_ids": node_ids, "edge_ids": edge_ids, "new_id": new_id, "status": status,
            "node_attrs": {k: np.asarray(v)[node_ids] for k, v in (node_attrs or {}).items()},
            "edge_attrs": {k: np.asarray(v)[edge_ids] for k, v in (edge_attrs or {}).items()}}


def undirected_degree(edge_index, n: int):
    """|{j : (i, j) in E or (j, i) in E}| per node, int32 [n]"""
    s, t = np.asarray(edge_index, np.int64).reshape(2, -1)
    pairs = np.unique(np.concatenate((np.stack((s, t), 1), np.stack((t, s), 1))), axis=0) if s.size else np.zeros((0, 2), np.int64)
    return np.bincount(pairs[:, 0], minlength=n).astype(np.int32)


def graphs_of(part: dict):
    """the graphs of an oracle result as ``Batch.to_data_list`` cuts them: [(edge_index local, node rows, edge rows)]"""
    out = []
    for g in range(len(part["ptr"]) - 1):
        n0, n1, e0, e1 = part["ptr"][g], part["ptr"][g + 1], part["edge_ptr"][g], part["edge_ptr"][g + 1]
        out.append({"edge_index": part["edge_index"][:, e0:e1] - n0,
                    "node_attrs": {k: v[n0:n1] for k, v in part["node_attrs"].items()},
                    "edge_attrs": {k: v[e0:e1] for k, v in part["edge_attrs"].items()}})
    return out


def random_batch(n: int, edges_per_node: float, n_graphs: int, seed: int, widths=(4,)):
    """a sound random batch: graph sizes from a multinomial (some may be empty), edges inside their graph, grouped by graph.
    -> dict: edge_index, batch, ptr, edge_ptr, x{w} float32 [n, w] per width, edge_attr float32 [E, 2]; NaNs with payloads in x"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = rng.multinomial(n, np.full(n_graphs, 1.0 / n_graphs)) if n else np.zeros(n_graphs, np.int64)
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    batch = np.repeat(np.arange(n_graphs), sizes).astype(np.int64)
    per = np.where(sizes > 0, np.floor(sizes * edges_per_node), 0).astype(np.int64)
    parts = [ptr[g] + rng.integers(0, sizes[g], size=(2, per[g])) for g in range(n_graphs) if per[g]]
    edge_index = np.concatenate(parts, axis=1).astype(np.int64) if parts else np.zeros((2, 0), np.int64)
    out = {"edge_index": edge_index, "batch": batch, "ptr": ptr, "edge_ptr": np.concatenate(([0], np.cumsum(per))).astype(np.int64),
           "edge_attr": rng.normal(size=(edge_index.shape[1], 2)).astype(np.float32)}
    for w in widths:
        bits = rng.integers(0, 2 ** 32, size=(n, w), dtype=np.uint64).astype(np.uint32)          # every bit pattern, NaN payloads included
        out[f"x{w}"] = bits.view(np.float32)
    return out


# ---- the hand-built cases --------------------------------------------------------------------------------------------
def hand_batch():
    """graph sizes (5, 0, 4, 1); the last graph has no edges"""
    sizes = [5, 0, 4, 1]
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    batch = np.repeat(np.arange(4), sizes)
    edge_index = np.array([[0, 1, 1, 2, 3, 4, 4, 0, 5, 6, 7, 8, 8, 6],
                           [1, 0, 2, 1, 4, 3, 0, 4, 6, 5, 8, 7, 6, 8]])
    return edge_index, batch, ptr


MASKS = {"all": (np.ones(10, bool), None), "none": (np.zeros(10, bool), None),
         "first": (np.array([0, 1, 1, 1, 1, 0, 1, 1, 1, 0], bool), None), "last": (np.array([1, 1, 1, 1, 0, 1, 1, 1, 0, 0], bool), None),
         "alternate": (np.arange(10) % 2 == 0, None), "edges": (None, np.arange(14) % 3 != 0),
         "both": (np.arange(10) % 4 != 1, np.arange(14) % 2 == 0)}


def bad_batch():
    """the hand batch with four unsound edges put in: an end at N, an end at -1, one joining two graphs, one out of graph order"""
    ei, batch, ptr = hand_batch()
    cols = ei.T.tolist()
    cols.insert(3, [2, 10])
    cols.insert(6, [-1, 3])
    cols.insert(9, [4, 5])
    cols.append([0, 1])                                       # graph 0 behind graph 2
    return np.array(cols).T, batch, ptr
