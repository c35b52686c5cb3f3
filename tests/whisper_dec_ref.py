"""float64 statement of the Whisper decoder and of greedy short-form generation (numpy only), written from the math:

    x = embed_tokens[id] + embed_positions[pos]
    per layer (pre-LN):  x += out(self_attn(LN1 x))          causal; q scaled by dh^-0.5; k_proj without bias
                         x += out(cross_attn(LN2 x, enc))    keys / values: k_proj / v_proj of the encoder's last state, no mask
                         x += fc2(gelu_erf(fc1(LN3 x)))
    logits = LN(x) . embed_tokens^T                          tied, no bias

and the generation loop of ``config.GenerationSpec``: prompt [start, language, task, no_timestamps], language by argmax over ``lang_ids``
of the step on [start] when not given, suppress_tokens at every generated position, begin_suppress_tokens at the first too, a row that has
emitted eos emits pad, stop when all rows have finished or the length reaches max_length.

tests/test_whisper_decoder_host.py pins it to HF's WhisperForConditionalGeneration (recorded in tests/golden/tiny_whisper_dec_d128h2.npz);
tests/test_gpu_whisper_decoder.py pins the device path to both.
"""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])


def enc_states(seed: int, B: int, T: int, D: int) -> np.ndarray:
    """The decoder fixture's encoder states: a per-utterance offset vector plus noise, fp32 [B, T, D] (numpy PCG64: the same on every host)."""
    g = np.random.default_rng(int(seed))
    off = g.standard_normal(size=(B, 1, D), dtype=np.float32)
    return (off + np.float32(0.5) * g.standard_normal(size=(B, T, D), dtype=np.float32)).astype(np.float32)


def _f64(sd, name):
    return np.asarray(sd[name], dtype=np.float64)


def layer_norm(x, sd, prefix, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * _f64(sd, prefix + ".weight") + _f64(sd, prefix + ".bias")


def linear(x, sd, prefix, bias=True):
    y = x @ _f64(sd, prefix + ".weight").T
    return y + _f64(sd, prefix + ".bias") if bias else y


def attend(q, K, V, heads):
    """q [D], K / V [n, D] -> [D]: per head softmax(q_h . K_h) V_h (q already scaled)."""
    D = q.shape[0]
    dh = D // heads
    out = np.empty(D)
    for h in range(heads):
        s = K[:, h * dh:(h + 1) * dh] @ q[h * dh:(h + 1) * dh]
        w = np.exp(s - s.max())
        out[h * dh:(h + 1) * dh] = (w / w.sum()) @ V[:, h * dh:(h + 1) * dh]
    return out


class Decoder:
    """One utterance: the cross keys / values once, then ``step(token, pos)`` -> logits over the vocabulary."""

    def __init__(self, geo, sd, enc):
        self.geo, self.sd = geo, sd
        self.L, self.H = geo.decoder_layers, geo.decoder_attention_heads
        self.scale = (geo.hidden // self.H) ** -0.5
        enc = np.asarray(enc, dtype=np.float64)
        self.cross = [(linear(enc, sd, f"decoder.layers.{i}.encoder_attn.k_proj", bias=False),
                       linear(enc, sd, f"decoder.layers.{i}.encoder_attn.v_proj")) for i in range(self.L)]
        self.k = [np.zeros((0, geo.hidden)) for _ in range(self.L)]
        self.v = [np.zeros((0, geo.hidden)) for _ in range(self.L)]

    def step(self, token: int, pos: int) -> np.ndarray:
        sd = self.sd
        assert pos == self.k[0].shape[0]
        x = _f64(sd, "decoder.embed_tokens.weight")[token] + _f64(sd, "decoder.embed_positions.weight")[pos]
        for i in range(self.L):
            p = f"decoder.layers.{i}"
            h = layer_norm(x, sd, p + ".self_attn_layer_norm")
            self.k[i] = np.vstack([self.k[i], linear(h, sd, p + ".self_attn.k_proj", bias=False)])
            self.v[i] = np.vstack([self.v[i], linear(h, sd, p + ".self_attn.v_proj")])
            x = x + linear(attend(linear(h, sd, p + ".self_attn.q_proj") * self.scale, self.k[i], self.v[i], self.H), sd, p + ".self_attn.out_proj")
            h = layer_norm(x, sd, p + ".encoder_attn_layer_norm")
            x = x + linear(attend(linear(h, sd, p + ".encoder_attn.q_proj") * self.scale, *self.cross[i], self.H), sd, p + ".encoder_attn.out_proj")
            h = layer_norm(x, sd, p + ".final_layer_norm")
            f = linear(h, sd, p + ".fc1")
            x = x + linear(0.5 * f * (1.0 + _erf(f / math.sqrt(2.0))), sd, p + ".fc2")
        return layer_norm(x, sd, "decoder.layer_norm") @ _f64(sd, "decoder.embed_tokens.weight").T


def masks(spec, V: int) -> np.ndarray:
    """[3, V] additive masks: steady, first generated position, language set."""
    m = np.zeros((3, V))
    m[0, list(spec.suppress_tokens)] = -np.inf
    m[1] = m[0]
    m[1, list(spec.begin_suppress_tokens)] = -np.inf
    m[2] = -np.inf
    m[2, list(spec.lang_ids)] = 0.0
    return m


def top2_margin(z: np.ndarray) -> float:
    a = np.sort(z)
    return float(a[-1] - a[-2])


def generate(geo, sd, spec, encs, language=None):
    """Greedy decoding of a batch in lock-step.  Returns dict(sequences [B, n] with prompt and eos / pad tail, languages [B], lists (ids
    after the prompt, up to and excluding eos), logits {(b, pos): raw logits of every DECIDED position}, margins {(b, pos): masked top-1 -
    top-2}); position p's logits decide token p + 1, p = 0 is the language step."""
    B, V = len(encs), geo.decoder_vocab_size
    m = masks(spec, V)
    dec = [Decoder(geo, sd, e) for e in encs]
    forced = {1: spec.task_id, 2: spec.no_timestamps_token_id}
    if language is not None:
        forced[0] = int(language)
    seq = [[spec.decoder_start_token_id] for _ in range(B)]
    done = [False] * B
    logits, margins = {}, {}
    pos = 0
    while len(seq[0]) < spec.max_length and not all(done):
        for b in range(B):
            z = dec[b].step(seq[b][pos], pos)
            if done[b]:
                tok = spec.pad_token_id
            elif pos in forced:
                tok = forced[pos]
            else:
                zm = z + m[2 if pos == 0 else 1 if pos == 3 else 0]
                tok = int(np.argmax(zm))
                logits[(b, pos)], margins[(b, pos)] = z, top2_margin(zm)
            seq[b].append(tok)
            if tok == spec.eos_token_id:
                done[b] = True
        pos += 1
    out = np.array(seq, dtype=np.int64)
    lists = []
    for b in range(B):
        gen = seq[b][spec.PROMPT_LEN:]
        lists.append(gen[:gen.index(spec.eos_token_id)] if spec.eos_token_id in gen else gen)
    return dict(sequences=out, languages=out[:, 1].copy(), lists=lists, logits=logits, margins=margins)


def teacher_forced(geo, sd, enc, ids) -> np.ndarray:
    """logits [len(ids), V] of one utterance fed ``ids`` position by position."""
    d = Decoder(geo, sd, enc)
    return np.stack([d.step(int(t), p) for p, t in enumerate(ids)])


def decided(seq, spec):
    """[(b, pos)] whose logits decide a token: the language step and every generated position of a row not yet finished."""
    out = []
    for b in range(seq.shape[0]):
        out.append((b, 0))
        for p in range(spec.PROMPT_LEN - 1, seq.shape[1] - 1):
            out.append((b, p))
            if seq[b, p + 1] == spec.eos_token_id:
                break
    return out


def gate(logits, seq, spec) -> float:
    """g = 1e-3 max(1, max|logits|) over the decided positions of a case (the project's gate)."""
    return 1e-3 * max(1.0, max(float(np.abs(logits[b, p]).max()) for b, p in decided(seq, spec)))


_FIXTURE = {}


def load_fixture(golden_dir):
    """(gold npz, geometry, decoder state dict, GenerationSpec, encoder states of case "a" [3, 1500, 128] fp32): weights and encoder states
    regenerated from the recorded seeds, checked against the recorded digest and probes.  Loaded once and shared; nobody writes to it."""
    if "v" not in _FIXTURE:
        import os
        from interspeech_ser_amd import config as C
        from interspeech_ser_amd.weights import state_dict_digest, synthetic_decoder_state_dict
        gold = np.load(os.path.join(golden_dir, "tiny_whisper_dec_d128h2.npz"))
        geo = C.TINY_WHISPER_DEC
        sd = synthetic_decoder_state_dict(geo, int(gold["decoder_seed"]))
        assert state_dict_digest(sd) == str(gold["digest"]), "the decoder weights are not the ones the fixture was recorded with"
        spec = C.GenerationSpec(
            decoder_start_token_id=int(gold["start"]), eos_token_id=int(gold["eos"]), pad_token_id=int(gold["pad"]),
            suppress_tokens=tuple(int(t) for t in gold["suppress"]), begin_suppress_tokens=tuple(int(t) for t in gold["begin_suppress"]),
            no_timestamps_token_id=int(gold["no_timestamps"]), lang_ids=tuple(int(t) for t in gold["lang_ids"]), task_id=int(gold["task"]),
            max_length=int(gold["max_length"]))
        enc = enc_states(int(gold["enc_seed"]), 3, geo.max_source_positions, geo.hidden)
        pr = gold["a_enc_probe_idx"]
        assert np.array_equal(enc[pr[:, 0], pr[:, 1], pr[:, 2]], gold["a_enc_probes"]), "the encoder states are not the recorded ones"
        _FIXTURE["v"] = (gold, geo, sd, spec, enc)
    return _FIXTURE["v"]
