"""Encoder time of the Parakeet int8 mode next to the f32 mode it is built on and the fp16 mode
(DESIGN.md §9.5): the full-size synthetic model on 64 x 1 s and 8 x 30 s, one process.
For each (shape, dtype): spt_parakeet_get_timings().encoder_ms (best of the calls after the first,
so graph-replayed where the shape repeats) and spt_parakeet_profile_encoder's per-stage split.
Usage: python scripts/pk_i8_measure.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.oracle import synth_audio  # noqa: E402
from spittle_amd import ParakeetEngine, ParakeetInferenceParams, ParakeetModelParams, TimestampGranularity  # noqa: E402

SPEC = "synthetic:parakeet-tdt-0.6b-v3"
SHAPES = (("64x1s", 64, 1.0), ("8x30s", 8, 30.0))


def main():
    out = {}
    prm = ParakeetInferenceParams(timestamp_granularity=TimestampGranularity.Token)
    for name, B, sec in SHAPES:
        pcms = [synth_audio(100 + b, int(16000 * sec)) for b in range(B)]
        for dt in ("i8", "f32", "f16"):
            e = ParakeetEngine()
            e.load_model_with_params(SPEC, ParakeetModelParams(dtype=dt, seed=7, max_batch=B, max_seconds=sec))
            enc = []
            for _ in range(4):
                e.transcribe_batch(pcms, prm)
                enc.append(e.timings()["encoder_ms"])
            rec = {"encoder_ms": min(enc[1:]), "encoder_ms_first": enc[0], "stages_ms": e.profile_encoder(3)}
            out[f"{name}/{dt}"] = rec
            print(name, dt, json.dumps(rec), flush=True)
            e.unload_model()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
