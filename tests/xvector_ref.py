"""The x-vector head of the hub's speaker-verification checkpoints, stated in float64 (numpy), and the helpers of its fixtures
(tests/golden/tiny_xvec_<family>.npz, written by tools/make_golden_xvector.py).  TEST INFRASTRUCTURE ONLY.

HF (modeling_wavlm.py WavLMForXVector.forward; the wav2vec2 / data2vec-audio / w2v-BERT classes are the same text), one utterance:
    hs = stack(hidden_states)                              [L+1, T, D]   (use_weighted_layer_sum; else the last state alone)
    x  = sum_l softmax(layer_weights)[l] * hs[l];   x = projector(x)
    per TDNN layer:  x[t] = relu(b + sum_j W_j x[t + j d]),  kernel.weight [out, k in] tap-major, T shrinks by d (k - 1)
    stats = cat(mean_t x, std_t x)  (unbiased);   embeddings = feature_extractor(stats);   logits = classifier(embeddings)
"""
from __future__ import annotations

import json
import os

import numpy as np

from audio_cls_ref import WRAPPER, softmax64, synth_wave            # noqa: F401  (one wave recipe, one wrapper table)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("tiny_xvec_wavlm", "tiny_xvec_wavlm_base", "tiny_xvec_w2v_bert")
MODES = ("f16x", "fp32x", "bf16")
N_PERTURB = 8


def _f(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def layer_mix(states, w) -> np.ndarray:
    """x[t, d] = ((w0 s0 + w1 s1) + w2 s2) + ... in float64, ascending state: the order ser_layer_mix_v states"""
    s = _f(states)
    out = _f(w)[0] * s[0]
    for l in range(1, s.shape[0]):
        out = out + _f(w)[l] * s[l]
    return out


def tdnn_layer(x, weight, bias, k: int, d: int) -> np.ndarray:
    """relu(b + sum_j W_j x[t + j d]) over the T - d (k - 1) full windows; ``weight`` [out, k * in], tap-major"""
    x, w = _f(x), _f(weight)
    T, C = x.shape
    Tn = T - d * (k - 1)
    assert Tn >= 1, (T, k, d)
    w = w.reshape(w.shape[0], k, C)
    y = np.tile(_f(bias)[None, :], (Tn, 1))
    for j in range(k):
        y = y + x[j * d: j * d + Tn] @ w[:, j, :].T
    return np.maximum(y, 0.0)


def stat_pool(x) -> np.ndarray:
    """cat(mean, unbiased std) over the rows, two-pass in float64"""
    x = _f(x)
    mean = x.mean(axis=0)
    return np.concatenate([mean, np.sqrt(((x - mean) ** 2).sum(axis=0) / (x.shape[0] - 1))])


def xvec_tail(stats, F, bf, Cw, bc):
    emb = _f(stats) @ _f(F).T + _f(bf)
    return emb, emb @ _f(Cw).T + _f(bc)


def tdnn_rows(states, head, weighted: bool, kernel, dilation) -> np.ndarray:
    """the last TDNN layer's rows [T', tdnn_dim[-1]] (after its ReLU) of one utterance from its hidden states [L+1, T, D]"""
    s = _f(states)
    x = layer_mix(s, softmax64(head["layer_weights"])) if weighted else s[-1]
    x = x @ _f(head["projector.weight"]).T + _f(head["projector.bias"])
    for i, (k, d) in enumerate(zip(kernel, dilation)):
        x = tdnn_layer(x, head[f"tdnn.{i}.kernel.weight"], head[f"tdnn.{i}.kernel.bias"], int(k), int(d))
    return x


def head_outputs(states, head, weighted: bool, kernel, dilation):
    """(float64 embeddings [dim], float64 logits [n]) of one utterance"""
    return xvec_tail(stat_pool(tdnn_rows(states, head, weighted, kernel, dilation)), head["feature_extractor.weight"],
                     head["feature_extractor.bias"], head["classifier.weight"], head["classifier.bias"])


def metric(a, b) -> float:
    """max|a - b| / max(1, max|b|)"""
    a, b = _f(a), _f(b)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


def gains(states, head, weighted: bool, kernel, dilation, eps: float, seed: int):
    """(embedding, logit) error by ``metric`` of the worst of N_PERTURB seeded sign patterns of size eps * max(1, max|hs|) added to the
    hidden states and pushed through the float64 statement"""
    s = _f(states)
    e0, l0 = head_outputs(s, head, weighted, kernel, dilation)
    size = eps * max(1.0, float(np.abs(s).max()))
    ge = gl = 0.0
    for i in range(N_PERTURB):
        sign = np.random.default_rng(seed * 100 + i).integers(0, 2, size=s.shape) * 2.0 - 1.0
        e, l = head_outputs(s + size * sign, head, weighted, kernel, dilation)
        ge, gl = max(ge, metric(e, e0)), max(gl, metric(l, l0))
    return ge, gl


class Fixture:
    """One tiny_xvec_<family>.npz: the HF config (JSON text), a preprocessor_config, the encoder's weights as (geometry, seed, digest) of
    ``weights.synthetic_state_dict``, the head tensors under HF names, six waveforms as (seed, length) of ``synth_wave`` -- index
    ``two`` gives T' = 2 exactly, index ``one`` T' = 1 (no expected output: it must fail alone), the others are ragged up to 1 s -- and
    per waveform with an output HF's float64 hidden states, ``embeddings`` and ``logits`` at batch size 1 (model in ``.double()``), and
    per mode the ``gain`` numbers of the end-to-end gate."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.name = name
        self.config = json.loads(str(z["config"]))
        self.preprocessor = json.loads(str(z["preprocessor"]))
        self.seed, self.digest = int(z["seed"]), str(z["digest"])
        self.lengths = [int(n) for n in z["lengths"]]
        self.wave_seeds = [int(s) for s in z["wave_seeds"]]
        self.two, self.one = int(z["two"]), int(z["one"])
        self.head = {k[5:]: np.asarray(z[k]) for k in z.files if k.startswith("head.")}
        self.good = [j for j in range(len(self.lengths)) if j != self.one]
        self.emb64 = {j: np.asarray(z[f"emb64_{j}"]) for j in self.good}
        self.logits64 = {j: np.asarray(z[f"logits64_{j}"]) for j in self.good}
        self.states64 = {j: np.asarray(z[f"states64_{j}"]) for j in self.good}
        self.gain_emb = {m: float(z[f"gain_emb_{m}"]) for m in MODES}
        self.gain_logits = {m: float(z[f"gain_logits_{m}"]) for m in MODES}
        self.weighted = bool(self.config.get("use_weighted_layer_sum", False))
        self.kernel, self.dilation = tuple(self.config["tdnn_kernel"]), tuple(self.config["tdnn_dilation"])

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
        return C.XVectorSpec.from_config(self.config, name=self.name)

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

    def outputs(self, j: int):
        return head_outputs(self.states64[j], self.head, self.weighted, self.kernel, self.dilation)
