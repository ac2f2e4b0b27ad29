"""Postprocessor.process_batch timed on the C2 batch shape (64 frames x 3000 nodes) and on one frame of it (MEASUREMENTS.md
row 3).  Positions: radargnn_amd.synthetic.radarscenes_frame; class probabilities: random logits through ops.softmax_rows;
random boxes; the thresholds of tests/test_gpu_postprocess.py::test_pipeline_loader_model_softmax_decode_nms.  One JSON line
per box width: median and spread (min, max) of --repeats host-clock timings with a device synchronise on both sides, after
--warmup calls, and a digest of the detections (the same on every commit that computes the same thing).  Uses only
process_batch, so it also runs on a checkout from before the segmented path, for the before / after pair; where
BoxSuppressor.apply_nms_frames exists, one frame is also timed through it (what keeps single frames on the single-frame
path).

    python tools/nms_frames_bench.py [--frames 64] [--repeats 30] [--warmup 3]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radargnn_amd import ops, postprocessor as P, synthetic  # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def digest(results):
    h = hashlib.sha1()
    for det, _ in results:
        for t in (det["boxes"].corners, det["scores"], det["labels"]):
            h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16], sum(len(det["boxes"]) for det, _ in results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    frames = [synthetic.radarscenes_frame(i) for i in range(args.frames)]
    pos = torch.from_numpy(np.concatenate([f.X for f in frames])).float().cuda()
    sizes = [f.X.shape[0] for f in frames]
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(sizes))), dtype=torch.int64).cuda()
    n = pos.shape[0]
    g = torch.Generator().manual_seed(0)
    prob = ops.softmax_rows((torch.randn(n, 6, generator=g) * 2).cuda())
    cfg = P.PostProcessingConfiguration(split="t", iou_for_nms=0.1, min_object_score={c: 0.05 for c in "abcde"},
                                        max_score_for_background=0.6, bg_index=5, bb_invariance="translation")
    segmented = hasattr(P.BoxSuppressor, "apply_nms_frames")
    for width in (5, 4):
        bb = torch.randn(n, width, generator=g)
        bb[:, 2:4] = bb[:, 2:4].abs() + 0.5
        if width == 5:
            bb[:, 4] = torch.rand(n, generator=g) * np.pi
        bb = bb.cuda()
        one = slice(0, sizes[0])
        batch = lambda: P.Postprocessor.process_batch(cfg, pos, bb, prob, ptr)                                  # noqa: E731
        single = lambda: P.Postprocessor.process_batch(cfg, pos[one], bb[one], prob[one], ptr[:2])              # noqa: E731
        results = batch()
        out = {"what": f"Postprocessor.process_batch, {args.frames} frames x {sizes[0]} nodes, box width {width}",
               "segmented_path": segmented, "repeats": args.repeats, "digest": digest(results)[0], "detections": digest(results)[1],
               "candidates": int(P.decode(prob, bb, pos, cfg)[2].sum()), "batch": timed(batch, args.repeats, args.warmup),
               "single_frame": timed(single, args.repeats, args.warmup), "single_frame_digest": digest(single())[0]}
        if segmented:
            label, score, keep, corners = P.decode(prob[one], bb[one], pos[one], cfg)
            seg = lambda: P.BoxSuppressor.apply_nms_frames(corners, score, label, keep, ptr[:2], cfg.iou_for_nms, width == 4)   # noqa: E731
            fin = lambda: P.Postprocessor._finish(cfg, pos[one], prob[one], label, score, keep, corners, width == 4)            # noqa: E731
            out["single_frame_suppression_segmented"] = timed(seg, args.repeats, args.warmup)
            out["single_frame_suppression_single_path"] = timed(fin, args.repeats, args.warmup)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
