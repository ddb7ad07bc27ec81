"""Host-side mirror of transcribe-rs' SenseVoiceEngine surface, over the spt_sensevoice_* C ABI.

Reference interface (transcribe-rs, as the app's TranscriptionManager uses it for the catalog entry
``sense-voice-int8``):
  * ``SenseVoiceEngine::new()`` + ``load_model_with_params(&path, SenseVoiceModelParams::int8())``
  * ``transcribe_samples(audio, Some(SenseVoiceInferenceParams { language, use_itn }))``; the app uses ``.text``
  * ``unload_model()``

``path`` is a synthetic spec (``"synthetic:sensevoice-small[:layers=a,b][:vocab=V][:seed=S]"``,
``sensevoice-test-small``; ``"empty:..."`` for weights supplied by load_state_dict / set_cmvn) or a
FunASR checkpoint directory (``model.pt``, ``am.mvn``, a SentencePiece ``.model`` or ``tokens.txt``),
read here in pure Python.  Everything below the boundary runs on the GPU; there is no CPU path.

[upstream, unverifiable offline] the ``am.mvn`` layout (Kaldi nnet text with ``<AddShift>`` and
``<Rescale>`` vectors) and the ``model.pt`` key names are recalled from FunASR, not checked against a
real checkpoint.
"""
from __future__ import annotations

import ctypes as C
import enum
import glob
import os
import re
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .engine import TranscriptionError, TranscriptionResult


class Language(enum.Enum):
    Auto = 0
    Chinese = 1
    English = 2
    Cantonese = 3
    Japanese = 4
    Korean = 5

    @staticmethod
    def from_code(code: str) -> "Language":
        """the app's selected_language -> Language (transcription.rs:518-525)"""
        return {"zh": Language.Chinese, "zh-Hans": Language.Chinese, "zh-Hant": Language.Chinese,
                "en": Language.English, "ja": Language.Japanese, "ko": Language.Korean,
                "yue": Language.Cantonese}.get(code, Language.Auto)


@dataclass
class SenseVoiceModelParams:
    dtype: str = "f16"            # the engine's only dtype
    device: int = 0
    max_batch: int = 8
    max_samples: int = 64 * 16000
    seed: int = 1234
    # recalled from FunASR, unverifiable offline: parameters with the recalled defaults
    ln_eps: float = 1e-5
    sanm_shift: int = 0
    lfr_m: int = 7
    lfr_n: int = 6
    blank_id: int = 0
    n_prefix: int = 4
    lang_rows: Tuple[int, ...] = (0, 3, 4, 7, 11, 12)
    event_row: int = 1
    emo_row: int = 2
    itn_row: int = 14
    no_itn_row: int = 15

    @staticmethod
    def int8() -> "SenseVoiceModelParams":
        """the app's constructor; the export's int8 arithmetic is not reproduced, the engine runs fp16"""
        return SenseVoiceModelParams()

    @staticmethod
    def fp32() -> "SenseVoiceModelParams":
        return SenseVoiceModelParams()


@dataclass
class SenseVoiceInferenceParams:
    language: Language = Language.Auto
    use_itn: bool = False


@dataclass
class SenseVoiceResult(TranscriptionResult):
    frames: List[int] = field(default_factory=list)   # row of each token's run start, 60 ms units
    prefix: List[int] = field(default_factory=list)   # language, emotion, event, ITN labels


_DT = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16, "i8": L.SPT_DTYPE_I8}


def read_am_mvn(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(neg_mean, inv_std) from a Kaldi-nnet text am.mvn: the bracketed vector after <AddShift> and
    the one after <Rescale>"""
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        text = f.read()
    out = []
    for tag in ("<AddShift>", "<Rescale>"):
        at = text.find(tag)
        m = re.search(r"\[([^\]]*)\]", text[at:]) if at >= 0 else None
        if not m:
            raise ValueError(f"{path}: no {tag} vector")
        try:
            out.append(np.array([float(v) for v in m.group(1).split()], np.float32))
        except ValueError:
            raise ValueError(f"{path}: the {tag} vector is not numeric") from None
    if out[0].size == 0 or out[0].size != out[1].size:
        raise ValueError(f"{path}: <AddShift> has {out[0].size} values, <Rescale> {out[1].size}")
    return out[0], out[1]


def _varint(b: bytes, at: int) -> Tuple[int, int]:
    v = s = 0
    while True:
        if at >= len(b) or s > 63:
            raise ValueError("truncated varint")
        c = b[at]
        at += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, at


def _pb_fields(b: bytes):
    at = 0
    while at < len(b):
        key, at = _varint(b, at)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            v, at = _varint(b, at)
        elif wt == 1:
            v, at = b[at:at + 8], at + 8
        elif wt == 2:
            n, at = _varint(b, at)
            if at + n > len(b):
                raise ValueError("truncated field")
            v, at = b[at:at + n], at + n
        elif wt == 5:
            v, at = b[at:at + 4], at + 4
        else:
            raise ValueError(f"unsupported wire type {wt}")
        yield fno, wt, v


def read_sentencepiece_pieces(path: str) -> List[str]:
    """pieces by id from a SentencePiece .model (ModelProto field 1 = repeated SentencePiece, whose field 1 is the piece)"""
    with open(path, "rb") as f:
        data = f.read()
    pieces = []
    try:
        for fno, wt, v in _pb_fields(data):
            if fno == 1 and wt == 2:
                piece = ""
                for f2, w2, v2 in _pb_fields(v):
                    if f2 == 1 and w2 == 2:
                        piece = v2.decode("utf-8", errors="replace")
                pieces.append(piece)
    except ValueError as e:
        raise ValueError(f"{path}: not a SentencePiece model ({e})") from None
    return pieces


def read_tokens_txt(path: str) -> List[str]:
    """pieces by id from tokens.txt: 'piece id' per line, or one piece per line in id order"""
    ids: Dict[int, str] = {}
    with open(path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f):
            line = line.rstrip("\r\n")
            parts = line.rsplit(" ", 1)
            if len(parts) == 2 and parts[1].isdigit():
                ids[int(parts[1])] = parts[0]
            else:
                ids[i] = line
    n = max(ids) + 1 if ids else 0
    return [ids.get(i, "") for i in range(n)]


def _check(lib, ctx, st):
    if st != L.SPT_OK:
        msg = lib.spt_sensevoice_last_error(ctx)
        raise TranscriptionError(st, msg.decode() if msg else "")


class SenseVoiceEngine:
    def __init__(self):
        self._lib = L.load()
        self._ctx = None
        self.model_spec: Optional[str] = None

    # ---- transcribe-rs surface
    def load_model_with_params(self, path: str, params: Optional[SenseVoiceModelParams] = None) -> None:
        params = params or SenseVoiceModelParams()
        self.unload_model()
        path = str(path)
        if path.startswith("synthetic:") or path.startswith("empty:"):
            self._create(path, params)
            return
        self.load_checkpoint_dir(path, params)

    def load_model(self, path: str) -> None:
        self.load_model_with_params(path, None)

    def load_checkpoint_dir(self, path: str, params: Optional[SenseVoiceModelParams] = None) -> None:
        """a FunASR SenseVoiceSmall directory: model.pt (torch.load, weights_only), am.mvn, and a
        SentencePiece .model or tokens.txt.  The geometry is read off the tensors' shapes."""
        params = params or SenseVoiceModelParams()
        pt = os.path.join(path, "model.pt")
        mvn = os.path.join(path, "am.mvn")
        if not os.path.isfile(pt) or not os.path.isfile(mvn):
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: neither a synthetic spec nor a FunASR checkpoint "
                                                     "directory (model.pt, am.mvn, a .model or tokens.txt)")
        import torch
        try:
            sd = torch.load(pt, map_location="cpu", weights_only=True)
        except Exception as e:  # a pickle that needs more than tensors
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{pt}: {e}") from None
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        sd = {k: v.detach().to(torch.float32).numpy() for k, v in sd.items() if hasattr(v, "detach")}
        try:
            d = int(sd["encoder.after_norm.weight"].shape[0])
            ff = int(sd["encoder.encoders0.0.feed_forward.w_1.weight"].shape[0])
            vocab = int(sd["ctc.ctc_lo.weight"].shape[0])
            width = int(sd["embed.weight"].shape[1])
        except KeyError as e:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{pt}: tensor {e} missing") from None
        count = lambda block: len({k.split(".")[2] for k in sd if k.startswith(f"encoder.{block}.")})  # noqa: E731
        n1, n2 = count("encoders"), count("tp_encoders")
        geo = {(512, 2048): "sensevoice-small", (256, 512): "sensevoice-test-small"}.get((d, ff))
        if geo is None or count("encoders0") != 1:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: unsupported geometry d={d} ff={ff}")
        if width != 80 * params.lfr_m:
            raise TranscriptionError(L.SPT_ERR_LOAD, f"{path}: embed width {width} is not 80 * lfr_m")
        try:
            neg_mean, inv_std = read_am_mvn(mvn)
        except ValueError as e:
            raise TranscriptionError(L.SPT_ERR_LOAD, str(e)) from None
        self._create(f"empty:{geo}:layers={n1},{n2}:vocab={vocab}", params)
        known = {k: v for k, v in sd.items() if self._numel_or_none(k) is not None}
        self.load_state_dict(known)
        self.set_cmvn(neg_mean, inv_std)
        sp = sorted(glob.glob(os.path.join(path, "*.model")))
        if sp:
            self.set_vocab(read_sentencepiece_pieces(sp[0]))
        elif os.path.isfile(os.path.join(path, "tokens.txt")):
            self.set_vocab(read_tokens_txt(os.path.join(path, "tokens.txt")))

    def unload_model(self) -> None:
        if self._ctx:
            self._lib.spt_sensevoice_destroy(self._ctx)
            self._ctx = None
            self.model_spec = None

    def is_loaded(self) -> bool:
        return self._ctx is not None

    def transcribe_samples(self, samples, params: Optional[SenseVoiceInferenceParams] = None) -> SenseVoiceResult:
        return self.transcribe_batch([samples], params)[0]

    def __del__(self):
        try:
            self.unload_model()
        except Exception:
            pass

    # ---- batched entry point, weights, introspection
    def transcribe_batch(self, batch: Sequence, params: Optional[SenseVoiceInferenceParams] = None) -> List[SenseVoiceResult]:
        ctx = self._need()
        arrs = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).ravel()) for x in batch]
        n = len(arrs)
        ptrs = C.cast((C.c_void_p * n)(*[a.ctypes.data for a in arrs]), C.POINTER(C.POINTER(C.c_float)))
        ns = (C.c_size_t * n)(*[a.size for a in arrs])
        outs = (C.POINTER(L.SvResult) * n)()
        ip = self._ip(params)
        _check(self._lib, ctx, self._lib.spt_sensevoice_transcribe_batch(ctx, ptrs, ns, n, C.byref(ip), outs))
        return [self._take(o) for o in outs]

    def load_state_dict(self, tensors: Dict[str, np.ndarray]) -> None:
        """FunASR state-dict names -> f32 arrays in FunASR's layout"""
        ctx = self._need()
        fp = C.POINTER(C.c_float)
        for name in tensors:
            a = np.ascontiguousarray(np.asarray(tensors[name], dtype=np.float32))
            _check(self._lib, ctx, self._lib.spt_sensevoice_set_tensor(ctx, name.encode(), a.ctypes.data_as(fp), a.size))

    def set_cmvn(self, neg_mean, inv_std) -> None:
        ctx = self._need()
        fp = C.POINTER(C.c_float)
        a = np.ascontiguousarray(np.asarray(neg_mean, dtype=np.float32).ravel())
        b = np.ascontiguousarray(np.asarray(inv_std, dtype=np.float32).ravel())
        if a.size != b.size:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, "CMVN vectors differ in length")
        _check(self._lib, ctx, self._lib.spt_sensevoice_set_cmvn(ctx, a.ctypes.data_as(fp), b.ctypes.data_as(fp), a.size))

    def set_vocab(self, pieces: Sequence[str]) -> None:
        ctx = self._need()
        enc = [p.encode("utf-8") for p in pieces]
        arr = (C.c_char_p * len(enc))(*enc)
        _check(self._lib, ctx, self._lib.spt_sensevoice_set_vocab(ctx, arr, len(enc)))

    def missing_tensors(self) -> int:
        return int(self._lib.spt_sensevoice_missing_tensors(self._need()))

    def tensor_numel(self, name: str) -> int:
        n = C.c_int64()
        _check(self._lib, self._need(), self._lib.spt_sensevoice_tensor_numel(self._need(), name.encode(), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        mi = L.SvModelInfo()
        _check(self._lib, self._need(), self._lib.spt_sensevoice_info(self._need(), C.byref(mi)))
        return {k: getattr(mi, k) for k, _ in L.SvModelInfo._fields_}

    def timings(self) -> dict:
        t = L.SvTimings()
        _check(self._lib, self._need(), self._lib.spt_sensevoice_get_timings(self._need(), C.byref(t)))
        return {k: getattr(t, k) for k, _ in L.SvTimings._fields_}

    def n_rows(self, n_samples: int) -> int:
        return int(self._lib.spt_sensevoice_n_rows(self._need(), int(n_samples)))

    # ---- test hooks
    def debug_features(self, samples) -> np.ndarray:
        ctx = self._need()
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).ravel())
        fp = C.POINTER(C.c_float)
        out = np.zeros((max(self.n_rows(x.size) - 4, 1), self.info()["input_dim"]), np.float32)
        _check(self._lib, ctx, self._lib.spt_sensevoice_debug_features(ctx, x.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp)))
        return out

    def debug_encode(self, samples, params: Optional[SenseVoiceInferenceParams] = None) -> np.ndarray:
        ctx = self._need()
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).ravel())
        fp = C.POINTER(C.c_float)
        out = np.zeros((max(self.n_rows(x.size), 1), self.info()["d"]), np.float32)
        ip = self._ip(params)
        _check(self._lib, ctx, self._lib.spt_sensevoice_debug_encode(ctx, x.ctypes.data_as(fp), x.size, C.byref(ip),
                                                                    out.ctypes.data_as(fp)))
        return out

    def debug_frames(self, samples, params: Optional[SenseVoiceInferenceParams] = None):
        """per encoder row: (top-1 id, top-1 logit, top-2 logit)"""
        ctx = self._need()
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).ravel())
        fp = C.POINTER(C.c_float)
        R = max(self.n_rows(x.size), 1)
        ids, t1, t2 = np.zeros(R, np.int32), np.zeros(R, np.float32), np.zeros(R, np.float32)
        ip = self._ip(params)
        _check(self._lib, ctx, self._lib.spt_sensevoice_debug_frames(
            ctx, x.ctypes.data_as(fp), x.size, C.byref(ip), ids.ctypes.data_as(C.POINTER(C.c_int32)),
            t1.ctypes.data_as(fp), t2.ctypes.data_as(fp)))
        return ids, t1, t2

    # ---- internals
    def _need(self):
        if not self._ctx:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, "model not loaded")
        return self._ctx

    def _numel_or_none(self, name: str) -> Optional[int]:
        n = C.c_int64()
        st = self._lib.spt_sensevoice_tensor_numel(self._need(), name.encode(), C.byref(n))
        return int(n.value) if st == L.SPT_OK else None

    @staticmethod
    def _ip(params: Optional[SenseVoiceInferenceParams]) -> "L.SvInferParams":
        p = params or SenseVoiceInferenceParams()
        lang = p.language.value if isinstance(p.language, Language) else int(p.language)
        return L.SvInferParams(int(lang), 1 if p.use_itn else 0)

    def _create(self, spec: str, params: SenseVoiceModelParams) -> None:
        if params.dtype not in _DT:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, f"bad dtype {params.dtype}")
        if len(params.lang_rows) != 6:
            raise TranscriptionError(L.SPT_ERR_INVALID_ARG, "lang_rows takes 6 rows")
        mp = L.SvModelParams(_DT[params.dtype], params.device, params.max_batch, params.max_samples, params.seed,
                             float(params.ln_eps), int(params.sanm_shift), int(params.lfr_m), int(params.lfr_n),
                             int(params.blank_id), int(params.n_prefix), (C.c_int32 * 6)(*[int(v) for v in params.lang_rows]),
                             int(params.event_row), int(params.emo_row), int(params.itn_row), int(params.no_itn_row))
        ctx = C.c_void_p()
        err = C.create_string_buffer(512)
        st = self._lib.spt_sensevoice_create(spec.encode(), C.byref(mp), C.byref(ctx), err, 512)
        if st != L.SPT_OK:
            raise TranscriptionError(st, err.value.decode(errors="replace"))
        self._ctx = ctx
        self.model_spec = spec

    def _take(self, o) -> SenseVoiceResult:
        try:
            r = o.contents
            n = r.n_tokens
            res = SenseVoiceResult(text=(r.text or b"").decode("utf-8", errors="replace"),
                                   tokens=[r.tokens[i] for i in range(n)],
                                   top1=np.array([r.top1[i] for i in range(n)], np.float32),
                                   top2=np.array([r.top2[i] for i in range(n)], np.float32),
                                   frames=[r.frames[i] for i in range(n)],
                                   prefix=[int(r.prefix[i]) for i in range(4)])
        finally:
            self._lib.spt_sensevoice_result_free(o)
        return res
