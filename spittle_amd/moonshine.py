"""Host-side mirror of transcribe-rs' MoonshineEngine surface, over the spt_moonshine_* C ABI.

Reference interface (transcribe-rs, as the app's TranscriptionManager uses it for the catalog entry
``moonshine-base``):
  * ``MoonshineEngine::new()`` + ``load_model_with_params(&path, MoonshineModelParams::variant(ModelVariant::Base))``
  * ``transcribe_samples(audio, None)`` -> ``TranscriptionResult``; the app uses ``.text``
  * ``unload_model()``

``path`` is a synthetic spec (``"synthetic:moonshine-base[:layers=N][:vocab=V][:eos=E][:seed=S]"``,
``moonshine-tiny``, ``moonshine-test-small``; ``"empty:..."`` for weights supplied by load_state_dict)
or an HF checkpoint directory (``config.json``, ``model.safetensors``, ``tokenizer.json``), read here
in pure Python / numpy.  Everything below the boundary runs on the GPU; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .engine import TranscriptionError, TranscriptionResult


class ModelVariant(enum.Enum):
    Tiny = "tiny"
    Base = "base"


@dataclass
class MoonshineModelParams:
    model_variant: ModelVariant = ModelVariant.Base
    dtype: str = "f16"            # the engine's only dtype
    device: int = 0
    max_batch: int = 8
    max_samples: int = 64 * 16000
    seed: int = 1234

    @staticmethod
    def variant(v) -> "MoonshineModelParams":
        return MoonshineModelParams(model_variant=ModelVariant(v.value if isinstance(v, ModelVariant) else str(v).lower()))


@dataclass
class MoonshineInferenceParams:
    tokens_per_second: float = 6.5
    max_tokens: int = 0           # > 0: the token limit itself


@dataclass
class MoonshineResult(TranscriptionResult):
    hit_eos: bool = False


_DT = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16, "i8": L.SPT_DTYPE_I8}
# geometry (d, heads, ff, layers) -> the engine's named models
_GEOMETRY = {(416, 8, 1664): "moonshine-base", (288, 8, 1152): "moonshine-tiny"}


def read_safetensors(path: str) -> Dict[str, np.ndarray]:
    """The safetensors container: u64 header length, a JSON header {name: {dtype, shape, data_offsets}},
    raw little-endian tensors.  F32 / F16 / BF16, returned as float32."""
    with open(path, "rb") as f:
        raw = f.read(8)
        if len(raw) != 8:
            raise ValueError(f"{path}: not a safetensors file")
        (hlen,) = struct.unpack("<Q", raw)
        size = os.path.getsize(path)
        if hlen > size - 8:
            raise ValueError(f"{path}: header length {hlen} past the end of the file")
        header = json.loads(f.read(hlen).decode("utf-8"))
        data = f.read()
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        b0, b1 = meta["data_offsets"]
        if not (0 <= b0 <= b1 <= len(data)):
            raise ValueError(f"{path}: tensor {name} outside the file")
        shape = tuple(int(s) for s in meta["shape"])
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        dt = meta["dtype"]
        if dt == "F32":
            a = np.frombuffer(data, "<f4", n, b0)
        elif dt == "F16":
            a = np.frombuffer(data, "<f2", n, b0).astype(np.float32)
        elif dt == "BF16":
            a = (np.frombuffer(data, "<u2", n, b0).astype(np.uint32) << 16).view(np.float32)
        else:
            raise ValueError(f"{path}: tensor {name} has unsupported dtype {dt}")
        if (b1 - b0) != n * (4 if dt == "F32" else 2):
            raise ValueError(f"{path}: tensor {name} size does not match its shape")
        out[name] = np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
    return out


def read_tokenizer_pieces(path: str) -> List[str]:
    """pieces by id from tokenizer.json: model.vocab ({piece: id} or [[piece, score], ...]) and added_tokens"""
    with open(path, "r", encoding="utf-8") as f:
        tk = json.load(f)
    vocab = tk.get("model", {}).get("vocab", {})
    ids = {}
    if isinstance(vocab, dict):
        ids = {int(i): p for p, i in vocab.items()}
    else:
        ids = {i: e[0] for i, e in enumerate(vocab)}
    for a in tk.get("added_tokens", []):
        ids[int(a["id"])] = a["content"]
    n = max(ids) + 1 if ids else 0
    return [ids.get(i, "") for i in range(n)]


def _check(lib, ctx, st):
    if st != L.SPT_OK:
        msg = lib.spt_moonshine_last_error(ctx)
        raise TranscriptionError(st, msg.decode() if msg else "")


class MoonshineEngine:
    def __init__(self):
        self._lib = L.load()
        self._ctx = None
        self.model_spec: Optional[str] = None

    # ---- transcribe-rs surface
    def load_model_with_params(self, path: str, params: Optional[MoonshineModelParams] = None) -> None:
        params = params or MoonshineModelParams()
        self.unload_model()
        path = str(path)
        if path.startswith("synthetic:") or path.startswith("empty:"):
            self._create(path, params)
            return
        cfg_path = os.path.join(path, "config.json")
        if not os.path.isfile(cfg_path):
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: neither a synthetic spec nor an HF checkpoint "
                                                     "directory (config.json, model.safetensors, tokenizer.json)")
        with open(cfg_path, "r", encoding="utf-8") as f:
            cfg = json.load(f)
        geo = (int(cfg["hidden_size"]), int(cfg.get("decoder_num_attention_heads", 8)), int(cfg["intermediate_size"]))
        if geo not in _GEOMETRY:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: unsupported geometry {geo}")
        want = "moonshine-" + params.model_variant.value
        if _GEOMETRY[geo] != want:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: a {_GEOMETRY[geo]} checkpoint, asked for {want}")
        n_enc, n_dec = int(cfg["encoder_num_hidden_layers"]), int(cfg["decoder_num_hidden_layers"])
        if n_enc != n_dec:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: {n_enc} encoder and {n_dec} decoder layers")
        spec = f"empty:{want}:layers={n_enc}:vocab={int(cfg['vocab_size'])}:eos={int(cfg.get('eos_token_id', 2))}"
        self._create(spec, params)
        self.load_state_dict(read_safetensors(os.path.join(path, "model.safetensors")))
        tok = os.path.join(path, "tokenizer.json")
        if os.path.isfile(tok):
            self.set_vocab(read_tokenizer_pieces(tok))

    def load_model(self, path: str) -> None:
        self.load_model_with_params(path, None)

    def unload_model(self) -> None:
        if self._ctx:
            self._lib.spt_moonshine_destroy(self._ctx)
            self._ctx = None
            self.model_spec = None

    def is_loaded(self) -> bool:
        return self._ctx is not None

    def transcribe_samples(self, samples, params: Optional[MoonshineInferenceParams] = None) -> MoonshineResult:
        return self.transcribe_batch([samples], params)[0]

    def __del__(self):
        try:
            self.unload_model()
        except Exception:
            pass

    # ---- batched entry point, weights, introspection
    def transcribe_batch(self, batch: Sequence, params: Optional[MoonshineInferenceParams] = None) -> List[MoonshineResult]:
        ctx = self._need()
        arrs = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).ravel()) for x in batch]
        n = len(arrs)
        ptrs = C.cast((C.c_void_p * n)(*[a.ctypes.data for a in arrs]), C.POINTER(C.POINTER(C.c_float)))
        ns = (C.c_size_t * n)(*[a.size for a in arrs])
        outs = (C.POINTER(L.MsResult) * n)()
        p = params or MoonshineInferenceParams()
        ip = L.MsInferParams(float(p.tokens_per_second), int(p.max_tokens))
        _check(self._lib, ctx, self._lib.spt_moonshine_transcribe_batch(ctx, ptrs, ns, n, C.byref(ip), outs))
        return [self._take(o) for o in outs]

    def load_state_dict(self, tensors: Dict[str, np.ndarray]) -> None:
        """HF state-dict names -> f32 arrays in HF's layout"""
        ctx = self._need()
        fp = C.POINTER(C.c_float)
        names = sorted(tensors, key=lambda k: k == "proj_out.weight")  # the tied tensor after the embedding
        for name in names:
            a = np.ascontiguousarray(np.asarray(tensors[name], dtype=np.float32))
            _check(self._lib, ctx, self._lib.spt_moonshine_set_tensor(ctx, name.encode(), a.ctypes.data_as(fp), a.size))

    def set_vocab(self, pieces: Sequence[str]) -> None:
        ctx = self._need()
        enc = [p.encode("utf-8") for p in pieces]
        arr = (C.c_char_p * len(enc))(*enc)
        _check(self._lib, ctx, self._lib.spt_moonshine_set_vocab(ctx, arr, len(enc)))

    def missing_tensors(self) -> int:
        return int(self._lib.spt_moonshine_missing_tensors(self._need()))

    def tensor_numel(self, name: str) -> int:
        n = C.c_int64()
        _check(self._lib, self._need(), self._lib.spt_moonshine_tensor_numel(self._need(), name.encode(), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        mi = L.MsModelInfo()
        _check(self._lib, self._need(), self._lib.spt_moonshine_info(self._need(), C.byref(mi)))
        return {k: getattr(mi, k) for k, _ in L.MsModelInfo._fields_}

    def timings(self) -> dict:
        t = L.MsTimings()
        _check(self._lib, self._need(), self._lib.spt_moonshine_get_timings(self._need(), C.byref(t)))
        return {k: getattr(t, k) for k, _ in L.MsTimings._fields_}

    # ---- test hooks
    def _frames(self, n: int) -> int:
        t1 = (n - 127) // 64 + 1
        return (((t1 - 7) // 3 + 1) - 3) // 2 + 1

    def debug_stem(self, samples, encoded: bool = False) -> np.ndarray:
        ctx = self._need()
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).ravel())
        fp = C.POINTER(C.c_float)
        out = np.zeros((max(self._frames(x.size), 1), self.info()["d"]), np.float32)
        fn = self._lib.spt_moonshine_debug_encode if encoded else self._lib.spt_moonshine_debug_stem
        _check(self._lib, ctx, fn(ctx, x.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp)))
        return out

    def debug_encode(self, samples) -> np.ndarray:
        return self.debug_stem(samples, encoded=True)

    def debug_logits(self, samples, prefix: Sequence[int]) -> np.ndarray:
        ctx = self._need()
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).ravel())
        pre = np.ascontiguousarray(np.asarray(prefix, dtype=np.int32))
        fp = C.POINTER(C.c_float)
        out = np.zeros((pre.size, self.info()["n_vocab"]), np.float32)
        _check(self._lib, ctx, self._lib.spt_moonshine_debug_logits(
            ctx, x.ctypes.data_as(fp), x.size, pre.ctypes.data_as(C.POINTER(C.c_int32)), pre.size, out.ctypes.data_as(fp)))
        return out

    # ---- internals
    def _need(self):
        if not self._ctx:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, "model not loaded")
        return self._ctx

    def _create(self, spec: str, params: MoonshineModelParams) -> None:
        if params.dtype not in _DT:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, f"bad dtype {params.dtype}")
        mp = L.MsModelParams(_DT[params.dtype], params.device, params.max_batch, params.max_samples, params.seed)
        ctx = C.c_void_p()
        err = C.create_string_buffer(512)
        st = self._lib.spt_moonshine_create(spec.encode(), C.byref(mp), C.byref(ctx), err, 512)
        if st != L.SPT_OK:
            raise TranscriptionError(st, err.value.decode(errors="replace"))
        self._ctx = ctx
        self.model_spec = spec

    def _take(self, o) -> MoonshineResult:
        try:
            r = o.contents
            n = r.n_tokens
            res = MoonshineResult(text=(r.text or b"").decode("utf-8", errors="replace"),
                                  tokens=[r.tokens[i] for i in range(n)],
                                  top1=np.array([r.top1[i] for i in range(n)], np.float32),
                                  top2=np.array([r.top2[i] for i in range(n)], np.float32),
                                  hit_eos=bool(r.hit_eos))
        finally:
            self._lib.spt_moonshine_result_free(o)
        return res
