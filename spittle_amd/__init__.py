"""spittle_amd -- MI355X-native (gfx950) Whisper, Parakeet-V3, Moonshine and SenseVoice transcription backend for Spittle.

The hot path (log-mel, encoder, cross-attention K/V, greedy decoder loop) is
hand-written HIP in spittle_amd/csrc, exported through the C ABI in
include/spittle_hip.h (libspittle_hip.so).  This package is the Python mirror of
the transcribe-rs WhisperEngine surface the app binds to.
"""
from .engine import (TranscriptionError, TranscriptionResult, TranscriptionSegment, WhisperEngine,
                     WhisperInferenceParams, WhisperModelParams)

from .parakeet import (ParakeetEngine, ParakeetInferenceParams, ParakeetModelParams, ParakeetResult,
                       TimestampGranularity)

from .moonshine import (ModelVariant, MoonshineEngine, MoonshineInferenceParams, MoonshineModelParams,
                        MoonshineResult)

from .sensevoice import (Language, SenseVoiceEngine, SenseVoiceInferenceParams, SenseVoiceModelParams,
                         SenseVoiceResult)

__all__ = ["Language", "ModelVariant", "MoonshineEngine", "MoonshineInferenceParams", "MoonshineModelParams",
           "MoonshineResult", "ParakeetEngine", "ParakeetInferenceParams", "ParakeetModelParams", "ParakeetResult",
           "SenseVoiceEngine", "SenseVoiceInferenceParams", "SenseVoiceModelParams", "SenseVoiceResult",
           "TimestampGranularity", "WhisperEngine", "WhisperInferenceParams", "WhisperModelParams", "TranscriptionResult",
           "TranscriptionSegment", "TranscriptionError"]
