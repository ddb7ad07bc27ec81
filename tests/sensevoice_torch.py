"""SenseVoice-Small in plain torch f32, restated from the issue's description of FunASR's SenseVoiceSmall
(no copy of FunASR is at hand: DESIGN.md §13 marks what is recalled): the Kaldi fbank, LFR + CMVN, the
query rows and positions, the SANM encoder, the CTC head and the greedy collapse as separate functions
over a dict of FunASR-named tensors.  The GPU tests' reference, and (emulate_f16=True) the model of
where the engine stores IEEE half: every matrix weight, every GEMM input, the fused q | k | v, the
attention's probabilities (its MFMA operand) and output, and the feed-forward's hidden activation;
the front end, the residual stream, the norms, the FSMN sum and the softmax are f32.

Also the seeded weights and audio the fixture and the GPU tests share."""
import math

import numpy as np
import torch
import torch.nn.functional as F

CASES = (400, 1360, 57999, 58000, 160000)   # samples: T = 1, 7, 360, 361, 998; R = 5, 6, 64, 65, 171
FIXTURE_LENGTHS = (400, 1360, 57999, 58000, 160000, 480000)
MEL_FLOOR = 1.192092955078125e-07
NQ = 4
LANG_ROWS = (0, 3, 4, 7, 11, 12)   # auto, zh, en, yue, ja, ko


class Dims:
    def __init__(self, d, heads, ff, n1, n2, vocab, lfr_m=7, lfr_n=6, shift=0, eps=1e-5, blank=0, n_prefix=4):
        self.d, self.H, self.ff, self.n0, self.n1, self.n2, self.vocab = d, heads, ff, 1, n1, n2, vocab
        self.dh = d // heads
        self.lfr_m, self.lfr_n, self.shift, self.eps, self.blank, self.n_prefix = lfr_m, lfr_n, shift, eps, blank, n_prefix
        self.inp = 80 * lfr_m


TEST_SMALL = Dims(256, 2, 512, 2, 1, 500)   # "sensevoice-test-small"
SMALL = Dims(512, 4, 2048, 49, 20, 25055)   # "sensevoice-small"
SPEC = "empty:sensevoice-test-small"
SEED = 42


def n_frames(n):
    return 0 if n < 400 else 1 + (n - 400) // 160


def n_lfr(T, lfr_n=6):
    return -(-T // lfr_n)


def n_rows(n, lfr_n=6):
    return n_lfr(n_frames(n), lfr_n) + NQ


def audio(n, seed):
    """three tones + noise at speech level, n samples"""
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    f = rng.uniform(100.0, 4000.0, 3)
    ph = rng.uniform(0.0, 2 * np.pi, 3)
    x = 0.1 * rng.standard_normal(n)
    t = np.arange(n) / 16000.0
    for k in range(3):
        x = x + 0.3 * np.sin(2 * np.pi * f[k] * t * (1.0 + 0.2 * np.sin(2 * np.pi * (k + 1) * t)) + ph[k])
    return np.clip(x, -1.0, 1.0).astype(np.float32)


# ---------------------------------------------------------------- front end
def mel_filters(dtype=torch.float32):
    """[257][80] Kaldi-scale filters, triangular in mel space, 20 Hz .. 8 kHz, no norm (f64, then cast)"""
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    pts = np.linspace(mel(20.0), mel(8000.0), 82)
    m = mel(np.arange(257) * (16000.0 / 512))[:, None]
    lo, ce, hi = pts[None, :-2], pts[None, 1:-1], pts[None, 2:]
    fb = np.maximum(0.0, np.minimum((m - lo) / (ce - lo), (hi - m) / (hi - ce)))
    return torch.from_numpy(fb).to(dtype)


def fbank(pcm, dtype=torch.float32):
    """Kaldi fbank [T][80] of float PCM in [-1, 1]: x 32768, snip_edges frames of 400 / 160, DC removal,
    pre-emphasis 0.97 (first sample x 0.03), symmetric Hamming, 512-point power spectrum, log mel"""
    x = torch.as_tensor(np.asarray(pcm, np.float32)).to(dtype) * 32768.0
    T = n_frames(x.numel())
    fr = x.unfold(0, 400, 160)[:T].clone()
    fr = fr - fr.mean(dim=1, keepdim=True)
    z = fr.clone()
    z[:, 1:] = fr[:, 1:] - 0.97 * fr[:, :-1]
    z[:, 0] = fr[:, 0] * (1.0 - 0.97)
    win = (0.54 - 0.46 * torch.cos(2.0 * math.pi * torch.arange(400, dtype=torch.float64) / 399.0)).to(dtype)
    spec = torch.fft.rfft(z * win, n=512)
    power = spec.real ** 2 + spec.imag ** 2
    return torch.log(torch.clamp(power @ mel_filters(dtype), min=MEL_FLOOR))


def lfr_index(T, m=7, n=6):
    """[T_lfr][m] frame indices: (m - 1) // 2 copies of frame 0 in front, the tail filled with the last frame"""
    i = torch.arange(n_lfr(T, n))[:, None] * n + torch.arange(m)[None, :] - (m - 1) // 2
    return i.clamp(0, T - 1)


def features(pcm, cmvn, D, dtype=torch.float32):
    """the LFR rows after CMVN [T_lfr][80 m]"""
    fb = fbank(pcm, dtype)
    rows = fb[lfr_index(fb.shape[0], D.lfr_m, D.lfr_n)].reshape(-1, D.inp)
    return (rows + cmvn[0].to(dtype)) * cmvn[1].to(dtype)


def positions(R, width):
    half = width // 2
    inc = math.log(10000.0) / (half - 1)
    inv = torch.exp(torch.arange(half, dtype=torch.float32) * -inc)
    ang = torch.arange(1, R + 1, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)


def input_rows(W, feats, D, language=0, use_itn=False):
    q = W["embed.weight"][[LANG_ROWS[language], 1, 2, 14 if use_itn else 15]]
    x = torch.cat([q, feats], dim=0) * math.sqrt(D.d)
    return x + positions(x.shape[0], D.inp)


# ---------------------------------------------------------------- encoder
def r16(x, on):
    return x.half().float() if on else x


def layer_prefix(D, l):
    if l < D.n0:
        return f"encoder.encoders0.{l}."
    if l < D.n0 + D.n1:
        return f"encoder.encoders.{l - D.n0}."
    return f"encoder.tp_encoders.{l - D.n0 - D.n1}."


def fsmn(v, w, shift=0):
    """v [R][d], w [d][1][11]: depthwise conv with 5 + shift zeros left, 5 - shift right, plus v"""
    R, d = v.shape
    vp = F.pad(v.t(), (5 + shift, 5 - shift))          # [d][R + 10]
    cols = vp.unfold(1, 11, 1)                          # [d][R][11]
    return (cols * w.reshape(d, 1, 11)).sum(dim=2).t() + v


def attention_core(q, k, v, H, emu=False):
    """softmax((q k^T) * dh^-0.5) v per head; emu: probabilities rounded to f16 for the PV product, the
    denominator summed from the unrounded ones, the output rounded to f16"""
    R, d = q.shape
    dh = d // H
    qh, kh, vh = (t.reshape(R, H, dh).transpose(0, 1) for t in (q, k, v))
    s = (qh @ kh.transpose(1, 2)) * (dh ** -0.5)
    p = torch.exp(s - s.max(dim=2, keepdim=True).values)
    o = (r16(p, emu) @ vh) / p.sum(dim=2, keepdim=True)
    return r16(o.transpose(0, 1).reshape(R, d), emu)


def encoder_layer(W, P, x, D, first, emu):
    d = D.d
    lin = lambda t, name: t @ r16(W[P + name + ".weight"], emu).t() + W[P + name + ".bias"]  # noqa: E731
    h = r16(F.layer_norm(x, (x.shape[1],), W[P + "norm1.weight"], W[P + "norm1.bias"], D.eps), emu)
    qkv = r16(lin(h, "self_attn.linear_q_k_v"), emu)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    mem = fsmn(v, W[P + "self_attn.fsmn_block.weight"], D.shift)
    att = attention_core(q, k, v, D.H, emu)
    x = (mem if first else x + mem) + lin(att, "self_attn.linear_out")
    h = r16(F.layer_norm(x, (d,), W[P + "norm2.weight"], W[P + "norm2.bias"], D.eps), emu)
    f = r16(F.relu(lin(h, "feed_forward.w_1")), emu)
    return x + lin(f, "feed_forward.w_2")


def encoder(W, x, D, emu=False):
    """input rows [R][80 m] -> the encoder output after tp_norm [R][d]"""
    for l in range(D.n0 + D.n1 + D.n2):
        x = encoder_layer(W, layer_prefix(D, l), x, D, l < D.n0, emu)
        if l == D.n0 + D.n1 - 1:
            x = F.layer_norm(x, (D.d,), W["encoder.after_norm.weight"], W["encoder.after_norm.bias"], D.eps)
    return F.layer_norm(x, (D.d,), W["encoder.tp_norm.weight"], W["encoder.tp_norm.bias"], D.eps)


def ctc_logits(W, enc, emu=False):
    return r16(enc, emu) @ r16(W["ctc.ctc_lo.weight"], emu).t() + W["ctc.ctc_lo.bias"]


def forward(W, cmvn, pcm, D, emu=False, language=0, use_itn=False):
    """(features, encoder output, logits)"""
    ft = features(pcm, cmvn, D)
    en = encoder(W, input_rows(W, ft, D, language, use_itn), D, emu)
    return ft, en, ctc_logits(W, en, emu)


def ctc_collapse(ids, n_prefix=4, blank=0):
    """(prefix labels, tokens, frames): runs of equal ids over rows n_prefix.. count once at their first
    row, blank runs dropped; frames count from n_prefix"""
    ids = [int(i) for i in ids]
    tok, frame = [], []
    for r in range(n_prefix, len(ids)):
        if r > n_prefix and ids[r] == ids[r - 1]:
            continue
        if ids[r] == blank:
            continue
        tok.append(ids[r])
        frame.append(r - n_prefix)
    return ids[:n_prefix], tok, frame


def margins(logits):
    t = np.sort(np.asarray(logits), axis=1)
    return t[:, -1] - t[:, -2]


# ---------------------------------------------------------------- seeded weights
def tensor_shapes(D):
    d, ff = D.d, D.ff
    s = {"embed.weight": (16, D.inp)}
    for l in range(D.n0 + D.n1 + D.n2):
        P = layer_prefix(D, l)
        din = D.inp if l < D.n0 else d
        s[P + "norm1.weight"] = s[P + "norm1.bias"] = (din,)
        s[P + "self_attn.linear_q_k_v.weight"], s[P + "self_attn.linear_q_k_v.bias"] = (3 * d, din), (3 * d,)
        s[P + "self_attn.fsmn_block.weight"] = (d, 1, 11)
        s[P + "self_attn.linear_out.weight"], s[P + "self_attn.linear_out.bias"] = (d, d), (d,)
        s[P + "norm2.weight"] = s[P + "norm2.bias"] = (d,)
        s[P + "feed_forward.w_1.weight"], s[P + "feed_forward.w_1.bias"] = (ff, d), (ff,)
        s[P + "feed_forward.w_2.weight"], s[P + "feed_forward.w_2.bias"] = (d, ff), (d,)
    for n in ("after_norm", "tp_norm"):
        s[f"encoder.{n}.weight"] = s[f"encoder.{n}.bias"] = (d,)
    s["ctc.ctc_lo.weight"], s["ctc.ctc_lo.bias"] = (D.vocab, d), (D.vocab,)
    return s


def make_weights(D, seed=SEED):
    """seeded numpy weights by FunASR name (sorted-name order): matrices N(0, 1 / fan_in), FSMN taps
    0.15 N, embed rows N(0, 1), norm weights 1 + 0.1 N, biases 0.02 N.  The CTC matrix is scaled so the
    logits spread with std about 8, and the blank bias is raised by 26 so blanks and repeats occur."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape in sorted(tensor_shapes(D).items()):
        g = rng.standard_normal(shape).astype(np.float32)
        if name.endswith(".bias"):
            w = 0.02 * g
        elif "norm" in name:
            w = 1.0 + 0.1 * g
        elif name == "embed.weight":
            w = g
        elif name.endswith("fsmn_block.weight"):
            w = 0.15 * g
        elif name == "ctc.ctc_lo.weight":
            w = g * (8.0 / math.sqrt(D.d))
        else:
            w = g / math.sqrt(shape[1])
        out[name] = np.ascontiguousarray(w.astype(np.float32))
    out["ctc.ctc_lo.bias"][D.blank] += 26.0
    return out


def make_cmvn(D, seed=SEED):
    """(neg_mean, inv_std) near the log-mel statistics of audio(): mean about 21, spread about 2.5"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    neg_mean = (-21.0 + 0.5 * rng.standard_normal(D.inp)).astype(np.float32)
    inv_std = (0.4 * (1.0 + 0.1 * rng.standard_normal(D.inp))).astype(np.float32)
    return neg_mean, inv_std


def to_torch(weights):
    return {k: torch.from_numpy(v) for k, v in weights.items()}
