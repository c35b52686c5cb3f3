"""Greedy CTC decoding stated in numpy, and the loader of its fixtures (tests/golden/tiny_ctc_<family>.npz, written by
tools/make_golden_ctc.py).  TEST INFRASTRUCTURE ONLY.

HF (modeling_wav2vec2.py Wav2Vec2ForCTC.forward; the HuBERT / WavLM / data2vec-audio / w2v-BERT classes are the same text), one utterance:
    logits = lm_head(last_hidden_state)            [T, V]
    predicted_ids = argmax(logits, -1)             [T]
    Wav2Vec2CTCTokenizer.decode: equal neighbours grouped, the groups of the pad token (the blank) dropped; char_offsets = each kept
    group's first frame and one past its last.
"""
from __future__ import annotations

import json
import os

import numpy as np

from audio_cls_ref import WRAPPER, synth_wave            # noqa: F401  (one wave recipe, one wrapper table)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("tiny_ctc_wavlm", "tiny_ctc_wavlm_base", "tiny_ctc_w2v_bert")
MODES = ("f16x", "fp32x", "bf16")


def frame_top2(z, V: int):
    """(ids int32 [T], margins fp32 [T], error flags [T]) of fp32 logits z [T, >= V]: columns >= V are not looked at; a NaN is read as
    +inf; the lowest index wins a tie; margin = top1 - top2 in ONE fp32 subtraction (+inf when V == 1); a frame whose winner is not finite
    is flagged."""
    x = np.array(np.asarray(z, dtype=np.float32)[:, :V], dtype=np.float32)
    x[np.isnan(x)] = np.inf
    ids = np.argmax(x, axis=1).astype(np.int32)                       # first occurrence of the maximum
    top1 = x[np.arange(x.shape[0]), ids]
    rest = x.copy()
    rest[np.arange(x.shape[0]), ids] = -np.inf
    top2 = rest.max(axis=1) if V > 1 else np.full(x.shape[0], -np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        margin = (top1.astype(np.float32) - top2.astype(np.float32)).astype(np.float32)
    return ids, margin, ~np.isfinite(top1)


def collapse(frame_ids, blank: int):
    """(ids, starts, ends) of one utterance's per-frame ids: frame t is kept when it is not the blank and differs from frame t - 1;
    ends[j] is one past the last frame of kept token j's run"""
    ids, starts, ends = [], [], []
    f = [int(t) for t in frame_ids]
    for t, tok in enumerate(f):
        if tok != blank and (t == 0 or tok != f[t - 1]):
            ids.append(tok)
            starts.append(t)
            e = t + 1
            while e < len(f) and f[e] == tok:
                e += 1
            ends.append(e)
    return ids, starts, ends


def greedy(z, frame_offs, V: int, blank: int):
    """The whole rule on packed ragged logits: dict(frame_ids, frame_margin, err, per utterance ids / starts / ends / min_margin)."""
    fid, margin, bad = frame_top2(z, V)
    out = dict(frame_ids=fid, frame_margin=margin, err=int(bad.any()), ids=[], starts=[], ends=[], min_margin=[])
    for b in range(len(frame_offs) - 1):
        r0, r1 = int(frame_offs[b]), int(frame_offs[b + 1])
        i, s, e = collapse(fid[r0:r1], blank)
        out["ids"].append(i)
        out["starts"].append(s)
        out["ends"].append(e)
        with np.errstate(invalid="ignore"):
            out["min_margin"].append(np.float32(np.fmin.reduce(margin[r0:r1])) if r1 > r0 else np.float32(np.inf))
    return out


def gate(logits64) -> float:
    """g = 1e-3 * max(1, max|logits|): the project's parity gate for a head's logits"""
    return 1e-3 * max(1.0, float(np.abs(np.asarray(logits64, dtype=np.float64)).max()))


def margins64(logits64) -> np.ndarray:
    s = np.sort(np.asarray(logits64, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


class Fixture:
    """One tiny_ctc_<family>.npz: the HF config (JSON text), a preprocessor_config, the encoder's weights as (geometry, seed, digest) of
    ``weights.synthetic_state_dict``, ``lm_head`` under HF names, the waveforms as (seed, length) of ``synth_wave`` -- the last one the
    shortest the stem admits (one frame) -- and per waveform HF's float64 logits at batch size 1 (model in ``.double()``), the per-frame
    ids, the collapsed ids and HF's char offsets in frames."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.name = name
        self.config = json.loads(str(z["config"]))
        self.preprocessor = json.loads(str(z["preprocessor"]))
        self.seed, self.digest, self.head_seed = int(z["seed"]), str(z["digest"]), int(z["head_seed"])
        self.lengths = [int(n) for n in z["lengths"]]
        self.wave_seeds = [int(s) for s in z["wave_seeds"]]
        self.head = {k[5:]: np.asarray(z[k]) for k in z.files if k.startswith("head.")}
        n = len(self.lengths)
        self.logits64 = [np.asarray(z[f"logits64_{j}"]) for j in range(n)]
        self.frame_ids = [np.asarray(z[f"frame_ids_{j}"]) for j in range(n)]
        self.ids = [[int(t) for t in z[f"ids_{j}"]] for j in range(n)]
        self.offsets = [[(int(s), int(e)) for s, e in np.asarray(z[f"offsets_{j}"]).reshape(-1, 2)] for j in range(n)]
        self.V, self.blank = int(self.config["vocab_size"]), int(self.config["pad_token_id"])

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
        return C.CTCSpec.from_config(self.config, name=self.name)

    def hf_state_dict(self):
        """The full state dict under the HF class's names: wrapper prefix + encoder tensors, and lm_head."""
        import torch
        from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
        geo = self.geometry()
        enc = synthetic_state_dict(geo, self.seed)
        assert state_dict_digest(enc) == self.digest, "the synthetic weight stream drifted from the one the fixture was made with"
        sd = {WRAPPER[geo.family] + k: v for k, v in enc.items()}
        sd.update({k: torch.from_numpy(np.array(v)) for k, v in self.head.items()})
        return sd

    def gate(self) -> float:
        """one g for the fixture, from the largest logit of any of its utterances"""
        return max(gate(l) for l in self.logits64)


def tiny_vocab(V: int, blank: int) -> dict:
    """token -> id for a V-entry test vocabulary: "<pad>" at ``blank``; "|", "<unk>" and then A, B, C, ... at the other ids in order"""
    names = ["|", "<unk>"] + [chr(ord("A") + i) for i in range(max(V, 2))]
    vocab, it = {}, iter(names)
    for i in range(V):
        vocab["<pad>" if i == blank else next(it)] = i
    return vocab
