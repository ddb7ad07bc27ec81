"""The fused cross-Q + cross-attention launch (dec_xq_fused) against the two-launch chain.

The fused launch runs the chain's instructions on the chain's operands: the cross-Q workgroups are
the stand-alone GEMV's, the attention workgroups take the q bits those stored, and the key blocks
are processed in the same order.  So every check here is bitwise: tokens, top-1 and top-2 of an
engine on the default path equal those of an engine created and run under SPT_XQ_FUSE=0.

  * eligible shapes (bf16 B = 8, bf16 B = 5: a partly filled row tile and 100 consumer workgroups,
    f16 B = 8) take the fused launch once per decoder layer of every one-token pass, no fallback;
  * ineligible shapes (B = 1, a beam-5 call, tiny.en in f32) never take it and match the chain too;
  * SPT_XQ_FUSE_FORCE_FALLBACK=1 makes the host treat a normal call as one whose consumers gave up:
    the rerun on the chain returns the same bits and counts one fallback (no wait runs out on the
    device here);
  * one run at the workload's depth (32 + 32 layers, bf16, B = 8).
"""
import contextlib
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 1234
LARGE22 = "synthetic:large-v3:enc=2:dec=2"
LARGE = "synthetic:large-v3"
TINY_EN = "synthetic:tiny.en"
N_STEPS = 16


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    kw.setdefault("no_timestamps", True)  # the device-resident greedy protocol (no fallback)
    kw.setdefault("temperature_inc", 0.0)
    kw.setdefault("ignore_eot", True)
    kw.setdefault("max_new_tokens", N_STEPS)
    return WhisperInferenceParams(**kw)


def _run(spec, dtype, B, fuse, force_fallback=False, n_utt=None, **kw):
    """One call of a fresh engine (max_batch B, n_utt or B utterances) -> (per-utterance (tokens, top1,
    top2), xq_stats, call_stats, info)."""
    from spittle_amd import WhisperEngine, WhisperModelParams
    with _env(SPT_XQ_FUSE=None if fuse else "0", SPT_XQ_FUSE_FORCE_FALLBACK="1" if force_fallback else None):
        e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=B, seed=SEED))
        e.load_model(spec)
        try:
            xs = [O.synth_audio(40 + i, 5 * 16000) for i in range(n_utt or B)]
            res = e.transcribe_batch(xs, _params(**kw))
            rows = [(list(r.tokens), np.asarray(r.top1).copy(), np.asarray(r.top2).copy()) for r in res]
            return rows, e.xq_stats(), e.call_stats(), e.info()
        finally:
            e.unload_model()


@pytest.fixture(scope="module")
def runs():
    """Each (spec, dtype, B, path) runs once; the tests share the results."""
    cache = {}

    def get(spec, dtype, B, fuse, **kw):
        key = (spec, dtype, B, fuse, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _run(spec, dtype, B, fuse, **kw)
        return cache[key]

    return get


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    for i, ((tk_a, t1_a, t2_a), (tk_b, t1_b, t2_b)) in enumerate(zip(a, b)):
        assert tk_a == tk_b, (what, i)
        assert np.array_equal(t1_a.view(np.uint32), t1_b.view(np.uint32)), (what, i)
        assert np.array_equal(t2_a.view(np.uint32), t2_b.view(np.uint32)), (what, i)


ELIGIBLE = [("bf16", 8), ("bf16", 5), ("f16", 8)]


@pytest.mark.parametrize("dtype,B", ELIGIBLE)
def test_fused_is_bitwise_the_chain(runs, dtype, B):
    fused, _, _, _ = runs(LARGE22, dtype, B, True)
    chain, xq, _, _ = runs(LARGE22, dtype, B, False)
    assert xq == {"fused_launches": 0, "fallbacks": 0}, xq  # SPT_XQ_FUSE=0 restores the chain
    assert all(len(r[0]) == N_STEPS and np.isfinite(r[1]).all() for r in fused)
    _same_bits(fused, chain, (dtype, B))


@pytest.mark.parametrize("dtype,B", ELIGIBLE)
def test_eligible_passes_take_the_fused_launch(runs, dtype, B):
    _, xq, cs, info = runs(LARGE22, dtype, B, True)
    one_token_passes = cs["decoder_passes"] - cs["engine_calls"]  # every pass but the prompt pass
    assert cs["engine_calls"] == 1 and one_token_passes == N_STEPS - 1, cs
    assert xq["fused_launches"] == one_token_passes * 2, (xq, cs)  # dec=2 layers
    assert xq["fallbacks"] == 0, xq
    assert cs["pd_passes"] == 0 and cs["pd_fallbacks"] == 0, cs


@pytest.mark.parametrize("spec,dtype,B,kw", [
    (LARGE22, "bf16", 1, {}),                                         # 20 workgroups: the 8-workgroup split
    (LARGE22, "bf16", 8, {"n_utt": 1, "beam_size": 5, "no_timestamps": False, "ignore_eot": False}),  # a beam's rows share a window
    (TINY_EN, "f32", 8, {}),                                          # f32, and a 4-wave cross-Q
], ids=["B1", "beam5", "tiny_f32"])
def test_ineligible_shapes_stay_on_the_chain(runs, spec, dtype, B, kw):
    dflt, xq, cs, _ = runs(spec, dtype, B, True, **kw)
    chain, xq0, _, _ = runs(spec, dtype, B, False, **kw)
    assert cs["decoder_passes"] > 1, cs
    assert xq == {"fused_launches": 0, "fallbacks": 0}, xq
    assert xq0 == {"fused_launches": 0, "fallbacks": 0}, xq0
    _same_bits(dflt, chain, (spec, dtype, B))


def test_forced_fallback_reruns_on_the_chain(runs):
    dflt, _, _, _ = runs(LARGE22, "bf16", 8, True)
    back, xq, _, _ = _run(LARGE22, "bf16", 8, True, force_fallback=True)
    assert xq["fallbacks"] == 1, xq
    assert xq["fused_launches"] == (N_STEPS - 1) * 2, xq  # the first attempt's; the rerun has none
    _same_bits(back, dflt, "forced fallback")


def test_full_depth_bitwise(runs):
    """32 decoder layers: every layer's tag, and the granule buffer reused by all of them."""
    fused, xq, cs, _ = runs(LARGE, "bf16", 8, True)
    chain, _, _, _ = runs(LARGE, "bf16", 8, False)
    assert xq == {"fused_launches": (N_STEPS - 1) * 32, "fallbacks": 0}, (xq, cs)
    _same_bits(fused, chain, "large-v3")
