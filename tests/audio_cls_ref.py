"""The head of the hub's audio-classification checkpoints, stated in float64 (numpy), and the helpers of its fixtures
(tests/golden/tiny_cls_<family>.npz, written by tools/make_golden_audio_cls.py).  TEST INFRASTRUCTURE ONLY.

HF (modeling_wavlm.py WavLMForSequenceClassification.forward; the wav2vec2 / HuBERT / data2vec-audio / w2v-BERT classes and
WhisperForAudioClassification are the same text):
    hs = stack(hidden_states)                              [L+1, T, D]   (use_weighted_layer_sum; else the last state alone)
    x  = sum_l softmax(layer_weights)[l] * hs[l]
    x  = projector(x);  p = mean over the frames of x;  out = classifier(p)
Here the mean is taken first: projector and mean are both linear, so mean_t(projector(x_t)) = projector(mean_t x_t).
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("tiny_cls_wavlm", "tiny_cls_wav2vec2", "tiny_cls_wavlm_base", "tiny_cls_w2v_bert", "tiny_cls_whisper")
HEAD_KEYS = ("projector.weight", "projector.bias", "classifier.weight", "classifier.bias", "layer_weights")
# the prefix the HF class puts in front of its encoder's parameter names
WRAPPER = {"wavlm": "wavlm.", "wav2vec2": "wav2vec2.", "hubert": "hubert.", "data2vec-audio": "data2vec_audio.",
           "wav2vec2-bert": "wav2vec2_bert.", "whisper": ""}


def softmax64(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float32).astype(np.float64)           # the fp32 parameter, then float64
    e = np.exp(v - v.max())
    return e / e.sum()


def layer_pool(states, w) -> np.ndarray:
    """pooled[d] = (1 / T) sum_t sum_l w[l] states[l, t, d] in float64; ``states`` [n, T, D], ``w`` [n]."""
    s = np.asarray(states, dtype=np.float64)
    return np.tensordot(np.asarray(w, dtype=np.float64), s, axes=(0, 0)).mean(axis=0)


def cls_tail(pooled, P, bp, Cw, bc) -> np.ndarray:
    f = lambda a: np.asarray(a, dtype=np.float64)                    # noqa: E731
    return (f(pooled) @ f(P).T + f(bp)) @ f(Cw).T + f(bc)


def head_logits(states, head, weighted: bool) -> np.ndarray:
    """float64 logits of one utterance from its hidden states [L+1, T, D]: pool first, then project and classify."""
    if weighted:
        pooled = layer_pool(states, softmax64(head["layer_weights"]))
    else:
        pooled = layer_pool(np.asarray(states)[-1:], np.ones(1))
    return cls_tail(pooled, head["projector.weight"], head["projector.bias"], head["classifier.weight"], head["classifier.bias"])


def synth_wave(seed: int, n: int) -> np.ndarray:
    """0.1 N(0, 1) + a 220 Hz sine at 0.2 + a DC offset of 0.05 (so that do_normalize changes the input), fp32 in [-1, 1]."""
    rng = np.random.default_rng(int(seed))
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.05 + 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


class Fixture:
    """One tiny_cls_<family>.npz: the HF config (JSON text), the encoder's weights as (geometry, seed, digest) of
    ``weights.synthetic_state_dict`` -- 1 MiB would not hold the tensors --, the five head tensors under HF names, three waveforms as
    (seed, length) of ``synth_wave``, and per waveform HF's logits at batch size 1 in fp32 and (model in ``.double()``) float64 with the
    float64 hidden states.  Whisper's states are 1 500 rows each, so that fixture keeps their float64 mean over the rows (``mean_j``,
    [L+1, 1, D]: for the head the same thing, rows being averaged anyway) and ``hs_absmax_j``."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.name = name
        self.config = json.loads(str(z["config"]))
        self.preprocessor = json.loads(str(z["preprocessor"]))
        self.seed, self.digest = int(z["seed"]), str(z["digest"])
        self.lengths = [int(n) for n in z["lengths"]]
        self.wave_seeds = [int(s) for s in z["wave_seeds"]]
        self.head = {k: np.asarray(z["head." + k]) for k in HEAD_KEYS if "head." + k in z.files}
        self.logits32 = [np.asarray(z[f"logits32_{j}"]) for j in range(len(self.lengths))]
        self.logits64 = [np.asarray(z[f"logits64_{j}"]) for j in range(len(self.lengths))]
        self.states64 = [np.asarray(z[f"states64_{j}"]) for j in range(len(self.lengths))]      # Whisper: [L+1, 1, D] row means
        self.hs_absmax = [float(z[f"hs_absmax_{j}"]) for j in range(len(self.lengths))]
        self.weighted = bool(self.config.get("use_weighted_layer_sum", False))

    def waves(self):
        return [synth_wave(s, n) for s, n in zip(self.wave_seeds, self.lengths)]

    def geometry(self):
        from interspeech_ser_amd import config as C
        geo = C.geometry_from_config(self.config, name=self.name)
        if geo.family == C.FAMILY_W2V_BERT:
            geo = C.replace(geo, fbank_mels=int(self.preprocessor["num_mel_bins"]), fbank_stride=int(self.preprocessor["stride"]))
        return geo

    def spec(self):
        from interspeech_ser_amd import config as C
        return C.ClassifierSpec.from_config(self.config, name=self.name)

    def hf_state_dict(self):
        """The full state dict under the HF class's names: wrapper prefix + encoder tensors, and the head's."""
        import torch
        from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
        geo = self.geometry()
        enc = synthetic_state_dict(geo, self.seed)
        assert state_dict_digest(enc) == self.digest, "the synthetic weight stream drifted from the one the fixture was made with"
        sd = {WRAPPER[geo.family] + k: v for k, v in enc.items()}
        sd.update({k: torch.from_numpy(np.array(v)) for k, v in self.head.items()})
        return sd

    def logit_bound(self, eps: float, j: int) -> np.ndarray:
        """Per-label bound of waveform j for a hidden-state error of eps * max(1, max|hs|): pooled is a convex combination of
        hidden-state rows, so |logit error| <= that * sum_d |(C P)[label, d]|."""
        cp = self.head["classifier.weight"].astype(np.float64) @ self.head["projector.weight"].astype(np.float64)
        return eps * max(1.0, self.hs_absmax[j]) * np.abs(cp).sum(axis=1)
