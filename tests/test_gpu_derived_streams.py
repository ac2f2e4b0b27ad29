"""Two streams drive one model while its weight-derived values (radargnn_amd.derived) are still being filled on the first."""
import pytest
import torch

from radargnn_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(not hasattr(torch.cuda, "_sleep"), reason="torch.cuda has no spin kernel to keep a stream's launches pending")
def test_second_stream_waits_for_folds_the_first_stream_is_still_filling():
    """Stream A's forward fills the per-module folds (folded update / edge / input-tail weights, summed biases, concatenated heads)
    behind a ~20 ms spin kernel, so its fill launches are still queued when stream B's forward hits the entries: every entry carries
    the event of its fill and B waits for it.  Both results equal the logits of a forward with fresh caches, bit for bit."""
    from radargnn_amd import derived, frames as fr, gnn, ops
    frames = [synthetic.radarscenes_frame(i, n_clusters=8, pts_per_cluster=20, n_clutter=140) for i in range(2)]
    g = fr.build_graphs(fr.FrameBatch.from_frames(frames), fr.GraphSettings(algorithm="radius", r=1.5))
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 64, 32], [6], [16, 5], True, True, [32, 64, 128, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(12)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    ops.invalidate_weight_caches()
    with torch.no_grad():
        c0, b0 = model(g.x, g.edge_index, g.edge_attr)
        assert "fold" in model.convs[0].__dict__[derived.HOLDER]          # (the forward under test takes the folded form)
        ops.invalidate_weight_caches()
        dev = g.x.device
        a, b = ops.independent_stream(dev), ops.independent_stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(a):
            torch.cuda._sleep(40_000_000)                                 # ~20 ms
            ca, ba = model(g.x, g.edge_index, g.edge_attr)
        with torch.cuda.stream(b):                                        # (no host synchronisation in between)
            cb, bb = model(g.x, g.edge_index, g.edge_attr)
        a.synchronize()
        b.synchronize()
    assert torch.equal(ca, c0) and torch.equal(ba, b0)
    assert torch.equal(cb, c0) and torch.equal(bb, b0)
