#!/usr/bin/env python
"""bf16 against fp32 edge MLP of the fused DualGNN path on the MI355X: the edge-score entry, its backward (stages 1 to
3) and the eval forward of a model with hidden 128, 4 layers, 4 heads.  The two precisions alternate inside every run;
three runs; per figure the median of the runs and their spread (max - min).  Times are HIP-event times of REPS calls
after a warm-up, in microseconds per call.  One JSON line per figure on stdout.

    python tools/bench_dual_bf16.py [--reps 20] [--runs 3]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))

from gnn._call import hip_call  # noqa: E402
from gnn.dual_gnn import DualGNN  # noqa: E402
from gnn.features import EDGE_FEATURE_DIM, NODE_FEATURE_DIM  # noqa: E402
from lap import _hip  # noqa: E402

DEV = torch.device("cuda:0")
HEADS = 4


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / reps


def edge_calls(B, N):
    lib = _hip.require_device()
    g = torch.Generator().manual_seed(1)
    layer = DualGNN(hidden_dim=128, layers=1, heads=HEADS).layers[0]
    edge = torch.randn((B, N, N, EDGE_FEATURE_DIM), generator=g).to(DEV)
    G = torch.randn((2 * HEADS, 128), generator=g).to(DEV) * 0.1
    w = [t.detach().to(DEV).contiguous() for t in (layer.edge_mlp[0].weight, layer.edge_mlp[0].bias,
                                                   layer.edge_mlp[3].weight, layer.edge_mlp[3].bias)]
    scores = torch.empty((B, 2 * HEADS, N, N), device=DEV)
    dS = torch.randn((B, 2 * HEADS, N, N), generator=g).to(DEV)
    grads = [torch.empty_like(t) for t in (*w, G)]
    ws = torch.empty((int(lib.lapwarm_dual_backward_workspace_bytes(B, N, HEADS)),), dtype=torch.uint8, device=DEV)
    head = (edge, *w, G)
    return {
        ("edge_scores", "fp32"): lambda: hip_call("lapwarm_dual_edge_scores", "bench", DEV, *head, scores, B, N, HEADS),
        ("edge_scores", "bf16"): lambda: hip_call("lapwarm_dual_edge_scores_bf16", "bench", DEV, *head, scores, None, B, N,
                                                  HEADS, 0, 0.0),
        ("edge_backward", "fp32"): lambda: hip_call("lapwarm_dual_edge_scores_backward", "bench", DEV, *head, dS, None,
                                                    *grads, B, N, HEADS, ws, ws.numel()),
        ("edge_backward", "bf16"): lambda: hip_call("lapwarm_dual_edge_scores_backward_bf16", "bench", DEV, *head, dS, None,
                                                    *grads, B, N, HEADS, ws, ws.numel(), 0, 0.0),
    }


def model_calls(B, N):
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=128, layers=4, heads=HEADS).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    edge = torch.randn((B, N, N, EDGE_FEATURE_DIM), generator=g).to(DEV)
    row, col = (torch.randn((B, N, NODE_FEATURE_DIM), generator=g).to(DEV) for _ in range(2))

    def call(precision):
        def run():
            model.fused_edge_precision = precision
            with torch.no_grad():
                model(edge, row, col)
        return run
    return {("model_forward", "fp32"): call("fp32"), ("model_forward", "bf16"): call("bf16")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    for B, N in ((1, 512), (1, 1024), (8, 256)):
        calls = {**edge_calls(B, N), **model_calls(B, N)}
        times = {key: [] for key in calls}
        for _ in range(a.runs):
            for what in ("edge_scores", "edge_backward", "model_forward"):
                for precision in ("bf16", "fp32"):  # alternating inside the run
                    times[(what, precision)].append(timed(calls[(what, precision)], a.reps))
        for what in ("edge_scores", "edge_backward", "model_forward"):
            rec = {"what": what, "B": B, "n": N}
            for precision in ("fp32", "bf16"):
                t = times[(what, precision)]
                rec[precision + "_us"] = round(statistics.median(t), 1)
                rec[precision + "_spread_us"] = round(max(t) - min(t), 1)
            rec["ratio"] = round(rec["fp32_us"] / rec["bf16_us"], 2)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
