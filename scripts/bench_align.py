"""DTW token timestamps at large-v3 bf16, B = 1: what the alignment adds to a call.  One JSON line.

On synthetic:large-v3 (seeded weights) one 30 s clip goes through the same whisper_full call with and
without the alignment (greedy, no timestamp tokens, no fallback, so both decode one window of
`--tokens` tokens), each warmed up and timed `--repeats` times (host clock around the call, which ends
in a device synchronise).  The line records both medians, their difference, the text tokens aligned,
and what the engine recorded of the alignment (spt_debug_align_stats): the replay's passes, the
alignment heads and the bytes of the alignment workspace.  The time inside align_qk, align_norm and
align_dtw needs a kernel trace (rocprofv3 --kernel-trace --stats around this script); the figures of
such a run are kept beside the line in profiles/align/kernel_trace.json.  --plain-only times the plain
call alone (the mode to compare against a tree without the alignment).  No device: the script fails.

    python scripts/bench_align.py [--repeats 10] [--warmup 3] [--tokens 64] [--plain-only] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "bench_line.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from oracle import oracle as O
    from spittle_amd import WhisperEngine, WhisperInferenceParams, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype="bf16", max_batch=1))
    e.load_model("synthetic:large-v3")
    x = O.synth_audio(0, 480000)
    prm = WhisperInferenceParams(language="en", no_timestamps=True, temperature_inc=0.0, max_new_tokens=a.tokens - 1)
    line = {"model": "synthetic:large-v3", "dtype": "bf16", "batch": 1, "audio_s": 30.0,
            "plain": timed(lambda: e.transcribe_samples(x, prm), a.warmup, a.repeats)}
    if not a.plain_only:
        r = e.transcribe_samples_aligned(x, prm)
        n = len(r.token_times)
        line["aligned"] = timed(lambda: e.transcribe_samples_aligned(x, prm), a.warmup, a.repeats)
        line["overhead_ms"] = line["aligned"]["median_ms"] - line["plain"]["median_ms"]
        line["text_tokens"] = n
        st = e.align_stats()  # as the engine recorded them (spt_debug_align_stats)
        line["replay_passes"] = st["replay_passes"]
        line["alignment_heads"] = st["alignment_heads"]
        line["workspace_bytes"] = st["workspace_bytes"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f)
        f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
