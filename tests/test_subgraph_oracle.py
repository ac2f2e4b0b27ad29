"""tests/subgraph_oracle.py against plain Python loops on hand-built graphs, and its hash against the literal values the header's
rule gives (computed with Python integers).  CPU only."""
import numpy as np
import pytest

import subgraph_oracle as S

MASK64 = 2 ** 64 - 1


def mix_int(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw_int(seed: int, s: int, t: int) -> int:
    lo, hi = min(s, t), max(s, t)
    return mix_int(mix_int(seed & MASK64) ^ (((lo << 32) & MASK64) | hi)) >> 40


DRAWS = [(0, 0, 1, 570621), (0, 1, 0, 570621), (1, 0, 1, 15334752), (12345, 7, 191999, 5680362),
         (-1, 2147483646, 3, 16769353), (2 ** 63 - 1, 5, 5, 4786746)]


def test_mix_literals():
    assert int(S.mix(0)) == 0xe220a8397b1dcdaf == mix_int(0)
    assert int(S.mix(1)) == 0x910a2dec89025cc1 == mix_int(1)


@pytest.mark.parametrize("seed,s,t,want", DRAWS)
def test_draw_literals(seed, s, t, want):
    assert draw_int(seed, s, t) == want
    assert int(S.pair_draw(seed, s, t)) == want
    assert int(S.pair_draw(seed, t, s)) == want


def test_kept_share_and_ends():
    rng = np.random.Generator(np.random.PCG64(5))
    pairs = rng.integers(0, 192000, size=(2, 200000))
    assert S.threshold(0.3) == 5033164 and S.threshold(0.0) == 0 and S.threshold(1.0) == 2 ** 24
    draws = S.pair_draw(99, pairs[0], pairs[1])
    assert np.array_equal(draws[:500], [draw_int(99, int(a), int(b)) for a, b in pairs.T[:500]])
    share = (draws >= S.threshold(0.3)).mean()
    assert abs(share - 0.7) < 5e-3, share                      # 200 000 Bernoulli draws: sigma = 0.001
    assert S.pair_mask(pairs, 192000, 99, 0.0).all() and not S.pair_mask(pairs, 192000, 99, 1.0).any()
    assert not S.pair_mask(np.array([[0, -1, 5], [5, 2, 0]]), 5, 99, 0.0).any()      # an end outside [0, n): never kept


# ---- the operation as loops ------------------------------------------------------------------------------------------
def loops(edge_index, batch, ptr, keep_nodes, keep_edges):
    n, e, b = len(batch), len(edge_index[0]), len(ptr) - 1
    new_id, count = [], 0
    for i in range(n):
        kept = keep_nodes is None or bool(keep_nodes[i])
        new_id.append(count if kept else -1)
        count += kept
    status, edges, edge_ids, per_graph = 0, [], [], [0] * b
    for k in range(e):
        s, t = int(edge_index[0][k]), int(edge_index[1][k])
        if not (0 <= s < n and 0 <= t < n):
            status |= S.BAD_ENDPOINT
            continue
        if not 0 <= batch[s] < b:
            status |= S.BAD_GRAPH
            continue
        if batch[s] != batch[t]:
            status |= S.CROSS_GRAPH
            continue
        if k > 0 and 0 <= edge_index[0][k - 1] < n and batch[edge_index[0][k - 1]] > batch[s]:
            status |= S.EDGE_ORDER
            continue
        if keep_edges is not None and not keep_edges[k]:
            continue
        if new_id[s] < 0 or new_id[t] < 0:
            continue
        edges.append((new_id[s], new_id[t]))
        edge_ids.append(k)
        per_graph[batch[s]] += 1
    new_ptr = [sum(1 for i in range(min(max(int(p), 0), n)) if new_id[i] >= 0) for p in ptr]
    edge_ptr = [sum(per_graph[:g]) for g in range(b + 1)]
    return new_id, edges, edge_ids, new_ptr, edge_ptr, status


@pytest.mark.parametrize("name", list(S.MASKS))
def test_oracle_equals_loops_on_the_hand_batch(name):
    ei, batch, ptr = S.hand_batch()
    kn, ke = S.MASKS[name]
    got = S.subgraph(ei, batch, ptr, kn, ke, node_attrs={"id": np.arange(10)}, edge_attrs={"id": np.arange(14)})
    new_id, edges, edge_ids, new_ptr, edge_ptr, status = loops(ei, batch, ptr, kn, ke)
    assert status == got["status"] == 0
    assert got["new_id"].tolist() == new_id and got["edge_ids"].tolist() == edge_ids
    assert got["edge_index"].T.tolist() == [list(p) for p in edges]
    assert got["ptr"].tolist() == new_ptr and got["edge_ptr"].tolist() == edge_ptr
    assert got["node_attrs"]["id"].tolist() == [i for i in range(10) if new_id[i] >= 0] == got["node_ids"].tolist()
    assert got["edge_attrs"]["id"].tolist() == edge_ids
    assert got["batch"].tolist() == [int(batch[i]) for i in got["node_ids"]]
    if name == "none":
        assert got["ptr"].tolist() == [0] * 5 and got["edge_index"].shape == (2, 0)


def test_oracle_equals_loops_on_bad_edges():
    ei, batch, ptr = S.bad_batch()
    for kn, ke in ((None, None), (np.arange(10) % 3 != 0, None), (None, np.arange(ei.shape[1]) % 2 == 0)):
        got = S.subgraph(ei, batch, ptr, kn, ke)
        new_id, edges, edge_ids, new_ptr, edge_ptr, status = loops(ei, batch, ptr, kn, ke)
        assert status == got["status"] == S.BAD_ENDPOINT | S.CROSS_GRAPH | S.EDGE_ORDER
        assert got["edge_ids"].tolist() == edge_ids and got["edge_index"].T.tolist() == [list(p) for p in edges]
        assert got["ptr"].tolist() == new_ptr and got["edge_ptr"].tolist() == edge_ptr
    sound = S.subgraph(*S.hand_batch())                          # without masks the sound edges are exactly the hand batch's
    assert np.array_equal(S.subgraph(ei, batch, ptr)["edge_index"], sound["edge_index"])
    assert S.subgraph(ei, np.where(batch == 3, 7, batch), ptr)["status"] & S.BAD_GRAPH == 0      # graph 3 has no edges
    assert S.subgraph(ei, np.where(batch == 2, 7, batch), ptr)["status"] & S.BAD_GRAPH


@pytest.mark.parametrize("seed", range(4))
def test_oracle_equals_loops_on_random_batches(seed):
    c = S.random_batch(60, 2.5, 5, seed)
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    kn, ke = rng.uniform(size=60) < 0.6, rng.uniform(size=c["edge_index"].shape[1]) < 0.7
    got = S.subgraph(c["edge_index"], c["batch"], c["ptr"], kn, ke)
    new_id, edges, edge_ids, new_ptr, edge_ptr, status = loops(c["edge_index"], c["batch"], c["ptr"], kn, ke)
    assert status == got["status"] == 0 and got["new_id"].tolist() == new_id
    assert got["edge_index"].T.tolist() == [list(p) for p in edges] and got["edge_ids"].tolist() == edge_ids
    assert got["ptr"].tolist() == new_ptr and got["edge_ptr"].tolist() == edge_ptr
    whole = S.subgraph(c["edge_index"], c["batch"], c["ptr"])
    assert np.array_equal(whole["edge_index"], c["edge_index"]) and np.array_equal(whole["edge_ptr"], c["edge_ptr"])


def test_degree_is_the_union_of_in_and_out_neighbours():
    ei = np.array([[0, 1, 0, 2, 3, 3], [1, 0, 2, 3, 2, 0]])
    want = [len({int(t) for s, t in ei.T if s == i} | {int(s) for s, t in ei.T if t == i}) for i in range(5)]
    assert S.undirected_degree(ei, 5).tolist() == want == [3, 1, 2, 2, 0]
    assert S.undirected_degree(np.zeros((2, 0), np.int64), 3).tolist() == [0, 0, 0]


def test_graphs_of_cuts_at_the_offsets():
    ei, batch, ptr = S.hand_batch()
    part = S.subgraph(ei, batch, ptr, S.MASKS["alternate"][0], None, node_attrs={"id": np.arange(10)})
    graphs = S.graphs_of(part)
    assert [len(g["node_attrs"]["id"]) for g in graphs] == [3, 0, 2, 0]
    assert graphs[0]["edge_index"].T.tolist() == [[2, 0], [0, 2]] and graphs[2]["edge_index"].T.tolist() == [[1, 0], [0, 1]]
