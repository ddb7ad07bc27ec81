"""Moonshine in plain torch f32, restated from HF transformers' modeling_moonshine.py: the PCM stem,
the encoder, the teacher-forced decoder and the greedy loop as separate functions over a dict of
HF-named tensors.  The GPU tests' reference, and (emulate_f16=True) the model of where the engine
stores IEEE half: weights of every matrix except conv1, every GEMM / GEMV input, q / k / v, the
encoder attention's probabilities (its MFMA operand) and each attention output; everything else f32.

Also the seeded weights and audio the fixtures and the GPU tests share (the fixtures store outputs,
not weights: both sides regenerate them from the seed)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

CASES = (895, 16000, 32077, 160000)  # samples: T3 = 1, 40, 82, 415


class Dims:
    def __init__(self, d, heads, ff, n_enc, n_dec, vocab, bos=1, eos=2, theta=10000.0):
        self.d, self.H, self.ff, self.n_enc, self.n_dec, self.vocab = d, heads, ff, n_enc, n_dec, vocab
        self.dh = d // heads
        self.rot = int(self.dh * 0.9)
        self.bos, self.eos, self.theta = bos, eos, theta


SMALL = Dims(416, 8, 1664, 2, 2, 1024)   # "moonshine-test-small": Base widths
TINY2 = Dims(288, 8, 1152, 2, 2, 1024)   # Tiny widths, 2 + 2 layers
# fixture name -> (dims, engine spec, weight seed, std of the 2-D tensors)
FIXTURES = {
    "moonshine_small": (SMALL, "empty:moonshine-test-small", 77, 0.035),
    "moonshine_tiny2": (TINY2, "empty:moonshine-tiny:layers=2:vocab=1024", 75, 0.035),
}


def frame_counts(n):
    t1 = (n - 127) // 64 + 1
    t2 = (t1 - 7) // 3 + 1
    t3 = (t2 - 3) // 2 + 1
    return t1, t2, t3


def max_tokens(n, tokens_per_second=6.5):
    return int(math.ceil(tokens_per_second * n / 16000.0))


def audio(n, seed):
    """tone + noise, as spittle_amd.synth.synth_audio, n samples"""
    rng = np.random.Generator(np.random.PCG64(3000 + seed))
    f = rng.uniform(100.0, 4000.0, 3)
    ph = rng.uniform(0.0, 2 * np.pi, 3)
    x = 0.1 * rng.standard_normal(n)
    t = np.arange(n) / 16000.0
    for k in range(3):
        x = x + 0.3 * np.sin(2 * np.pi * f[k] * t + ph[k])
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def tensor_shapes(D):
    """every tensor of MoonshineForConditionalGeneration(cfg).state_dict() but the tied proj_out.weight"""
    d, ff = D.d, D.ff
    s = {"model.encoder.conv1.weight": (d, 1, 127), "model.encoder.groupnorm.weight": (d,),
         "model.encoder.groupnorm.bias": (d,), "model.encoder.conv2.weight": (2 * d, d, 7),
         "model.encoder.conv2.bias": (2 * d,), "model.encoder.conv3.weight": (d, 2 * d, 3),
         "model.encoder.conv3.bias": (d,), "model.encoder.layer_norm.weight": (d,),
         "model.decoder.embed_tokens.weight": (D.vocab, d), "model.decoder.norm.weight": (d,)}
    for l in range(D.n_enc):
        p = f"model.encoder.layers.{l}."
        for n in "qkvo":
            s[p + f"self_attn.{n}_proj.weight"] = (d, d)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (ff, d), (ff,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (d, ff), (d,)
        s[p + "input_layernorm.weight"] = s[p + "post_attention_layernorm.weight"] = (d,)
    for l in range(D.n_dec):
        p = f"model.decoder.layers.{l}."
        for a in ("self_attn", "encoder_attn"):
            for n in "qkvo":
                s[p + f"{a}.{n}_proj.weight"] = (d, d)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (2 * ff, d), (2 * ff,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (d, ff), (d,)
        for n in ("input_layernorm", "post_attention_layernorm", "final_layernorm"):
            s[p + n + ".weight"] = (d,)
    return s


def make_weights(D, seed, std):
    """seeded numpy weights by HF name (sorted-name order): matrices and convolutions N(0, std^2)
    (conv1: N(0, 0.1^2), its fan-in is one channel), norm weights 1 + 0.1 N, biases 0.02 N"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape in sorted(tensor_shapes(D).items()):
        g = rng.standard_normal(shape).astype(np.float32)
        if name.endswith("norm.weight"):
            w = 1.0 + 0.1 * g
        elif name.endswith(".bias"):
            w = 0.02 * g
        elif name.endswith("conv1.weight"):
            w = 0.1 * g
        else:
            w = std * g
        out[name] = np.ascontiguousarray(w.astype(np.float32))
    return out


def to_torch(weights):
    return {k: torch.from_numpy(v) for k, v in weights.items()}


def r16(x, on):
    return x.half().float() if on else x


def _ln(x, w):
    return F.layer_norm(x, (x.shape[-1],), w, None, 1e-5)


def _rope_tables(D, positions):
    inv = 1.0 / (D.theta ** (torch.arange(0, D.rot, 2, dtype=torch.float) / D.rot))
    ang = positions.float()[:, None] * inv[None, :]
    return ang.cos(), ang.sin()  # [T][rot / 2]


def _rope(x, cos, sin, rot):
    """x [T][H][dh]: interleaved pairs of the first rot dims rotated"""
    xr, xp = x[..., :rot], x[..., rot:]
    a, b = xr[..., 0::2], xr[..., 1::2]
    c, s = cos[:, None, :], sin[:, None, :]
    o = torch.stack((a * c - b * s, b * c + a * s), dim=-1).flatten(-2)
    return torch.cat((o, xp), dim=-1)


def _attend(q, k, v, D, mask, emu, round_p):
    """q [Tq][H][dh], k / v [Tk][H][dh] (already rounded) -> [Tq][d]"""
    s = torch.einsum("qhe,khe->hqk", q, k) * (D.dh ** -0.5)
    if mask is not None:
        s = s + mask
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    o = torch.einsum("hqk,khe->qhe", r16(p, emu and round_p), v) / l.permute(1, 0, 2)
    return r16(o.reshape(q.shape[0], D.d), emu)


def stem(W, pcm, D, emulate_f16=False):
    e = emulate_f16
    x = torch.as_tensor(pcm, dtype=torch.float32)[None, None, :]
    h = torch.tanh(F.conv1d(x, W["model.encoder.conv1.weight"], None, stride=64))
    h = F.group_norm(h, 1, W["model.encoder.groupnorm.weight"], W["model.encoder.groupnorm.bias"], 1e-5)
    h = F.gelu(F.conv1d(r16(h, e), r16(W["model.encoder.conv2.weight"], e), W["model.encoder.conv2.bias"], stride=3))
    h = F.gelu(F.conv1d(r16(h, e), r16(W["model.encoder.conv3.weight"], e), W["model.encoder.conv3.bias"], stride=2))
    return h[0].T.contiguous()  # [T3][d]


def encoder(W, x, D, emulate_f16=False):
    e = emulate_f16
    T = x.shape[0]
    cos, sin = _rope_tables(D, torch.arange(T))
    for l in range(D.n_enc):
        p = f"model.encoder.layers.{l}."
        xn = r16(_ln(x, W[p + "input_layernorm.weight"]), e)
        q, k, v = (xn @ r16(W[p + f"self_attn.{n}_proj.weight"], e).T for n in "qkv")
        q = r16(_rope(q.view(T, D.H, D.dh), cos, sin, D.rot), e)
        k = r16(_rope(k.view(T, D.H, D.dh), cos, sin, D.rot), e)
        v = r16(v.view(T, D.H, D.dh), e)
        x = x + _attend(q, k, v, D, None, e, True) @ r16(W[p + "self_attn.o_proj.weight"], e).T
        xn = r16(_ln(x, W[p + "post_attention_layernorm.weight"]), e)
        h = r16(F.gelu(xn @ r16(W[p + "mlp.fc1.weight"], e).T + W[p + "mlp.fc1.bias"]), e)
        x = x + h @ r16(W[p + "mlp.fc2.weight"], e).T + W[p + "mlp.fc2.bias"]
    return _ln(x, W["model.encoder.layer_norm.weight"])


def decoder_logits(W, enc, tokens, D, emulate_f16=False):
    """teacher-forced: logits [len(tokens)][V], row s from tokens[0..s]"""
    e = emulate_f16
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long)
    T, Te = tok.shape[0], enc.shape[0]
    emb = r16(W["model.decoder.embed_tokens.weight"], e)
    x = emb[tok]
    cos, sin = _rope_tables(D, torch.arange(T))
    causal = torch.full((T, T), float("-inf")).triu(1)[None]
    enc16 = r16(enc, e)
    for l in range(D.n_dec):
        p = f"model.decoder.layers.{l}."
        xn = r16(_ln(x, W[p + "input_layernorm.weight"]), e)
        q, k, v = (xn @ r16(W[p + f"self_attn.{n}_proj.weight"], e).T for n in "qkv")
        q = r16(_rope(q.view(T, D.H, D.dh), cos, sin, D.rot), e)
        k = r16(_rope(k.view(T, D.H, D.dh), cos, sin, D.rot), e)
        v = r16(v.view(T, D.H, D.dh), e)
        x = x + _attend(q, k, v, D, causal, e, False) @ r16(W[p + "self_attn.o_proj.weight"], e).T
        xn = r16(_ln(x, W[p + "post_attention_layernorm.weight"]), e)
        q = r16(xn @ r16(W[p + "encoder_attn.q_proj.weight"], e).T, e).view(T, D.H, D.dh)
        k = r16(enc16 @ r16(W[p + "encoder_attn.k_proj.weight"], e).T, e).view(Te, D.H, D.dh)
        v = r16(enc16 @ r16(W[p + "encoder_attn.v_proj.weight"], e).T, e).view(Te, D.H, D.dh)
        x = x + _attend(q, k, v, D, None, e, False) @ r16(W[p + "encoder_attn.o_proj.weight"], e).T
        xn = r16(_ln(x, W[p + "final_layernorm.weight"]), e)
        y = xn @ r16(W[p + "mlp.fc1.weight"], e).T + W[p + "mlp.fc1.bias"]
        h, gate = y.chunk(2, dim=-1)
        g = r16(F.silu(gate) * h, e)
        x = x + g @ r16(W[p + "mlp.fc2.weight"], e).T + W[p + "mlp.fc2.bias"]
    return r16(_ln(x, W["model.decoder.norm.weight"]), e) @ emb.T


def greedy(W, enc, D, n_max, emulate_f16=False):
    """argmax decoding from [bos]: the tokens (eos not included), whether eos ended it, and the logits rows"""
    toks, rows = [D.bos], []
    for _ in range(n_max):
        lg = decoder_logits(W, enc, toks, D, emulate_f16)[-1]
        rows.append(lg)
        t = int(lg.argmax())
        if t == D.eos:
            return toks[1:], True, torch.stack(rows)
        toks.append(t)
    return toks[1:], False, torch.stack(rows) if rows else torch.zeros(0, D.vocab)


def margins(logits):
    """top-1 minus top-2 of each row"""
    t = torch.as_tensor(logits).topk(2, dim=-1).values
    return (t[:, 0] - t[:, 1]).numpy()


def fixture_rows(t3):
    """the rows of the stem / encoder output a fixture stores (all of a short one, 24 spread over a long one)"""
    return np.unique(np.round(np.linspace(0, t3 - 1, min(t3, 24))).astype(np.int64))
