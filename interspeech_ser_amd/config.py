"""Encoder geometries for the SSL embedding-extraction path.

The reference never spells these numbers out: it calls
``AutoModel.from_pretrained(--ssl_type)`` (preprocess_speech.py:111-114,
preprocess_whisper.py:119-122) and the hub ``config.json`` supplies them.
SURVEY.md section 8a cross-checks the values below against parameter counts and
the ``feat1_dim`` entries of the reference's configs/*.json.

A geometry is a plain dataclass so that the CPU oracle (oracle/) can consume it
by attribute access without importing this package.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

FAMILY_WAVLM = "wavlm"
FAMILY_WAV2VEC2 = "wav2vec2"
FAMILY_HUBERT = "hubert"
FAMILY_WHISPER = "whisper"
FAMILY_ROBERTA = "roberta"      # text side of the bimodal heads (next row 8f-1)
FAMILY_DEBERTA = "deberta"      # DeBERTa-v2/v3 variant of the text side (engine.DebertaEncoder, csrc/deberta.hip)
FAMILY_DATA2VEC_AUDIO = "data2vec-audio"   # layer-norm conv stem, post-LN encoder, a stack of LayerNorm'd positional convs
FAMILY_W2V_BERT = "wav2vec2-bert"          # Kaldi fbank front end, conformer layers with a relative-key attention bias (engine.W2vBertEncoder)
# wav2vec2's conv stem, conformer layers with rotary or Transformer-XL relative positions, a centred BatchNorm convolution module
# (engine.ConformerSpeechEncoder)
FAMILY_W2V_CONFORMER = "wav2vec2-conformer"

SPEECH_FAMILIES = (FAMILY_WAVLM, FAMILY_WAV2VEC2, FAMILY_HUBERT, FAMILY_DATA2VEC_AUDIO)
W2V_CONFORMER_POSITION_TYPES = ("rotary", "relative")


@dataclass(frozen=True)
class EncoderGeometry:
    family: str
    num_layers: int
    hidden: int
    heads: int
    ffn: int
    # wav2vec2-style convolutional waveform encoder (all three speech families)
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    feat_proj_layer_norm: bool = True      # HuBERT makes this optional
    # the *-base checkpoints (HF config defaults): GroupNorm(C, C) over time after conv layer 0 and no norm after layers 1..6
    # ("group"), post-LayerNorm encoder layers (stable_layer_norm False); the *-large / xlarge / XLS-R ones: "layer", True
    feat_extract_norm: str = "layer"
    stable_layer_norm: bool = True
    pos_conv_kernel: int = 128
    pos_conv_groups: int = 16
    # positional embedding: ONE weight-normed grouped conv + GELU ("weight": wavlm / wav2vec2 / hubert), or a stack of pos_conv_layers
    # plain grouped convs, each followed by a non-affine LayerNorm and GELU ("layer": data2vec-audio, HF Data2VecAudioPositionalConvLayer)
    pos_conv_layers: int = 1
    pos_conv_norm: str = "weight"
    # WavLM gated relative position bias
    num_buckets: int = 320
    max_bucket_distance: int = 800
    layer_norm_eps: float = 1e-5
    # Whisper encoder
    n_mels: int = 128
    max_source_positions: int = 1500
    # RoBERTa text encoder
    vocab_size: int = 50265
    max_positions: int = 514
    pad_token_id: int = 1
    type_vocab_size: int = 1
    # DeBERTa-v2/v3 disentangled attention (log-bucketed relative positions, shared q/k projections for positions)
    position_buckets: int = 256
    # DeBERTa-v2 xlarge / xxlarge: ConvLayer after encoder layer 0 (HF modeling_deberta_v2.py ConvLayer; 0 = none, as in v3)
    text_conv_kernel: int = 0
    # w2v-BERT 2.0 (HF Wav2Vec2BertModel): stacked log-mel rows in (fbank_mels x fbank_stride = feature_projection_input_dim), the causal
    # depthwise kernel of the conformer convolution module, and the clamp of the relative-key distance embedding
    fbank_mels: int = 80
    fbank_stride: int = 2
    conv_depthwise_kernel: int = 31
    left_max_positions: int = 64
    right_max_positions: int = 8
    # wav2vec2-conformer (HF Wav2Vec2ConformerModel): "rotary" or "relative" (Transformer-XL); "" for every other family.  ``rotary_base``:
    # rotary_embedding_base.  (``max_source_positions`` above is also this family's key: the length HF pre-computes its relative table for;
    # the table here grows with the longest utterance, so the value is recorded and nothing reads it.)
    position_type: str = ""
    rotary_base: int = 10000
    name: str = ""

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    # Whisper decoder (engine.WhisperDecoder): attached by ``with_decoder``, read through the properties below.  It is deliberately not a
    # dataclass field: an encoder geometry compares, hashes and round-trips through a checkpoint's config.json as it did before the
    # decoder was described (the encoder-only consumers never look at it).  ``dataclasses.replace`` drops it; ``with_decoder`` re-attaches.
    @property
    def decoder(self) -> Optional["DecoderGeometry"]:
        return self.__dict__.get("_decoder")

    @property
    def decoder_layers(self) -> int:
        return self.decoder.layers if self.decoder else 0

    @property
    def decoder_attention_heads(self) -> int:
        return self.decoder.attention_heads if self.decoder else 0

    @property
    def decoder_ffn_dim(self) -> int:
        return self.decoder.ffn_dim if self.decoder else 0

    @property
    def decoder_vocab_size(self) -> int:
        return self.decoder.vocab_size if self.decoder else 0

    @property
    def max_target_positions(self) -> int:
        return self.decoder.max_target_positions if self.decoder else 448

    @property
    def num_hidden_states(self) -> int:
        return self.num_layers + 1

    def frames_for(self, num_samples: int) -> int:
        """Integer frame count of the conv stack: floor((L-k)/s)+1 per layer
        (HF modeling_wavlm.py:633-652).  Bit-exact gate of SURVEY 8a row a8."""
        n = int(num_samples)
        if self.family == FAMILY_W2V_BERT:
            # 400-sample frames every 160 (center=False), stacked fbank_stride at a time; HF's extra masked row of an odd count is not a row here
            return max(0, 1 + (n - 400) // 160) // self.fbank_stride if n >= 400 else 0
        for k, s in zip(self.conv_kernel, self.conv_stride):
            n = (n - k) // s + 1
        return n

    @property
    def fbank_dim(self) -> int:
        return self.fbank_mels * self.fbank_stride

    @property
    def distance_positions(self) -> int:
        return self.left_max_positions + self.right_max_positions + 1

    def frame_chain(self, num_samples: int):
        out = []
        n = int(num_samples)
        for k, s in zip(self.conv_kernel, self.conv_stride):
            n = (n - k) // s + 1
            out.append(n)
        return out


@dataclass(frozen=True)
class DecoderGeometry:
    """The decoder of a Whisper checkpoint (config.json: decoder_layers, decoder_attention_heads, decoder_ffn_dim, vocab_size,
    max_target_positions); the model width is the encoder's ``hidden``."""
    layers: int
    attention_heads: int
    ffn_dim: int
    vocab_size: int
    max_target_positions: int = 448


def with_decoder(geo: EncoderGeometry, layers: int, attention_heads: int, ffn_dim: int, vocab_size: int,
                 max_target_positions: int = 448) -> EncoderGeometry:
    """A copy of a Whisper geometry that also describes the checkpoint's decoder."""
    g = replace(geo)
    object.__setattr__(g, "_decoder", DecoderGeometry(int(layers), int(attention_heads), int(ffn_dim), int(vocab_size), int(max_target_positions)))
    return g


WAVLM_LARGE = EncoderGeometry(
    family=FAMILY_WAVLM, num_layers=24, hidden=1024, heads=16, ffn=4096,
    conv_bias=False, name="microsoft/wavlm-large")

XLSR_2B = EncoderGeometry(
    family=FAMILY_WAV2VEC2, num_layers=48, hidden=1920, heads=16, ffn=7680,
    conv_bias=True, name="facebook/wav2vec2-xls-r-2b")

HUBERT_XLARGE = EncoderGeometry(
    family=FAMILY_HUBERT, num_layers=48, hidden=1280, heads=16, ffn=5120,
    conv_bias=True, feat_proj_layer_norm=True,
    name="facebook/hubert-xlarge-ls960-ft")

WHISPER_LARGE_V3 = with_decoder(EncoderGeometry(
    family=FAMILY_WHISPER, num_layers=32, hidden=1280, heads=20, ffn=5120,
    n_mels=128, max_source_positions=1500, name="openai/whisper-large-v3"), 32, 20, 5120, 51866, 448)

ROBERTA_LARGE = EncoderGeometry(
    family=FAMILY_ROBERTA, num_layers=24, hidden=1024, heads=16, ffn=4096, name="roberta-large")

# deberta-v3: DebertaV2Config(position_buckets=256, share_att_key, pos_att_type p2c|c2p, norm_rel_ebd layer_norm,
# position_biased_input False, type_vocab_size 0, layer_norm_eps 1e-7, pad_token_id 0, vocab 128100)
DEBERTA_V3_LARGE = EncoderGeometry(
    family=FAMILY_DEBERTA, num_layers=24, hidden=1024, heads=16, ffn=4096, vocab_size=128100, max_positions=512,
    pad_token_id=0, type_vocab_size=0, layer_norm_eps=1e-7, position_buckets=256, name="microsoft/deberta-v3-large")
DEBERTA_V3_BASE = EncoderGeometry(
    family=FAMILY_DEBERTA, num_layers=12, hidden=768, heads=12, ffn=3072, vocab_size=128100, max_positions=512,
    pad_token_id=0, type_vocab_size=0, layer_norm_eps=1e-7, position_buckets=256, name="microsoft/deberta-v3-base")

# deberta-v2-xlarge is what the reference's README runs preprocess_deroberta.py with (README.md:66): the v3 attention
# settings plus conv_kernel_size = 3, conv_act = "gelu" (a token-axis Conv1d of the embeddings added to layer 0's output)
DEBERTA_V2_XLARGE = EncoderGeometry(
    family=FAMILY_DEBERTA, num_layers=24, hidden=1536, heads=24, ffn=6144, vocab_size=128100, max_positions=512,
    pad_token_id=0, type_vocab_size=0, layer_norm_eps=1e-7, position_buckets=256, text_conv_kernel=3,
    name="microsoft/deberta-v2-xlarge")
DEBERTA_V2_XXLARGE = EncoderGeometry(
    family=FAMILY_DEBERTA, num_layers=48, hidden=1536, heads=24, ffn=6144, vocab_size=128100, max_positions=512,
    pad_token_id=0, type_vocab_size=0, layer_norm_eps=1e-7, position_buckets=256, text_conv_kernel=3,
    name="microsoft/deberta-v2-xxlarge")

# the base checkpoints: transformers' WavLMConfig() / Wav2Vec2Config() / HubertConfig() defaults (GroupNorm stem, post-LN encoder)
WAVLM_BASE = EncoderGeometry(
    family=FAMILY_WAVLM, num_layers=12, hidden=768, heads=12, ffn=3072, conv_bias=False,
    feat_extract_norm="group", stable_layer_norm=False, name="microsoft/wavlm-base")
WAVLM_BASE_PLUS = replace(WAVLM_BASE, name="microsoft/wavlm-base-plus")
WAV2VEC2_BASE = EncoderGeometry(
    family=FAMILY_WAV2VEC2, num_layers=12, hidden=768, heads=12, ffn=3072, conv_bias=False,
    feat_extract_norm="group", stable_layer_norm=False, name="facebook/wav2vec2-base")
HUBERT_BASE = EncoderGeometry(
    family=FAMILY_HUBERT, num_layers=12, hidden=768, heads=12, ffn=3072, conv_bias=False,
    feat_extract_norm="group", stable_layer_norm=False, name="facebook/hubert-base-ls960")

# data2vec-audio: layer-norm conv stem, post-LN encoder, positional embedding = 5 x [grouped Conv1d(k 19, pad 9, 16 groups) -> LayerNorm
# (no affine) -> GELU].  Base = transformers' Data2VecAudioConfig() defaults; large = 1024 / 24 / 16 / 4096 with the same stem and
# positional stack.  Written from the public hub configs, which cannot be fetched offline to be checked here: a snapshot's config.json
# takes precedence over these entries (resolve_geometry).
DATA2VEC_AUDIO_BASE = EncoderGeometry(
    family=FAMILY_DATA2VEC_AUDIO, num_layers=12, hidden=768, heads=12, ffn=3072, conv_bias=False, stable_layer_norm=False,
    pos_conv_kernel=19, pos_conv_groups=16, pos_conv_layers=5, pos_conv_norm="layer", name="facebook/data2vec-audio-base")
DATA2VEC_AUDIO_LARGE = EncoderGeometry(
    family=FAMILY_DATA2VEC_AUDIO, num_layers=24, hidden=1024, heads=16, ffn=4096, conv_bias=False, stable_layer_norm=False,
    pos_conv_kernel=19, pos_conv_groups=16, pos_conv_layers=5, pos_conv_norm="layer", name="facebook/data2vec-audio-large")

# w2v-BERT 2.0: transformers' Wav2Vec2BertConfig() defaults are the checkpoint's (24 conformer layers, 16 heads of 64, 600 M parameters)
W2V_BERT_2 = EncoderGeometry(
    family=FAMILY_W2V_BERT, num_layers=24, hidden=1024, heads=16, ffn=4096, fbank_mels=80, fbank_stride=2, conv_depthwise_kernel=31,
    left_max_positions=64, right_max_positions=8, layer_norm_eps=1e-5, name="facebook/w2v-bert-2.0")

# wav2vec2-conformer large (fairseq's conformer models, LV-60 pre-training; the -960h-ft fine-tunes share the encoder): the wav2vec2-large
# stem (layer norm, conv bias), 24 conformer layers, K = 31.  Written from the public hub configs, which cannot be fetched offline to be
# checked here: a snapshot's config.json takes precedence over these entries (resolve_geometry).
W2V_CONFORMER_ROPE_LARGE = EncoderGeometry(
    family=FAMILY_W2V_CONFORMER, num_layers=24, hidden=1024, heads=16, ffn=4096, conv_bias=True, feat_extract_norm="layer",
    conv_depthwise_kernel=31, position_type="rotary", rotary_base=10000, max_source_positions=5000,
    name="facebook/wav2vec2-conformer-rope-large")
W2V_CONFORMER_REL_LARGE = replace(W2V_CONFORMER_ROPE_LARGE, position_type="relative", name="facebook/wav2vec2-conformer-rel-pos-large")

_REGISTRY = {
    "microsoft/deberta-v3-large": DEBERTA_V3_LARGE,
    "microsoft/deberta-v2-xlarge": DEBERTA_V2_XLARGE,
    "microsoft/deberta-v2-xxlarge": DEBERTA_V2_XXLARGE,
    "microsoft/deberta-v3-base": DEBERTA_V3_BASE,
    "roberta-large": ROBERTA_LARGE,
    "FacebookAI/roberta-large": ROBERTA_LARGE,
    "microsoft/wavlm-large": WAVLM_LARGE,
    "wavlm-large": WAVLM_LARGE,                       # the reference's argparse default
    "facebook/wav2vec2-xls-r-2b": XLSR_2B,
    "facebook/hubert-xlarge-ls960-ft": HUBERT_XLARGE,
    "facebook/hubert-xlarge-ll60k": HUBERT_XLARGE,
    "openai/whisper-large-v3": WHISPER_LARGE_V3,
    "microsoft/wavlm-base": WAVLM_BASE,             # "wavlm-base": the reference's organiser baseline (suffix rule of geometry_for)
    "microsoft/wavlm-base-plus": WAVLM_BASE_PLUS,
    "microsoft/wavlm-base-plus-sv": replace(WAVLM_BASE, name="microsoft/wavlm-base-plus-sv"),
    "facebook/wav2vec2-base": WAV2VEC2_BASE,
    "facebook/hubert-base-ls960": HUBERT_BASE,
    "facebook/data2vec-audio-base": DATA2VEC_AUDIO_BASE,
    "facebook/data2vec-audio-base-960h": replace(DATA2VEC_AUDIO_BASE, name="facebook/data2vec-audio-base-960h"),
    "facebook/data2vec-audio-large": DATA2VEC_AUDIO_LARGE,
    "facebook/data2vec-audio-large-960h": replace(DATA2VEC_AUDIO_LARGE, name="facebook/data2vec-audio-large-960h"),
    "facebook/w2v-bert-2.0": W2V_BERT_2,
    "facebook/wav2vec2-conformer-rope-large": W2V_CONFORMER_ROPE_LARGE,
    "facebook/wav2vec2-conformer-rope-large-960h-ft": replace(W2V_CONFORMER_ROPE_LARGE, name="facebook/wav2vec2-conformer-rope-large-960h-ft"),
    "facebook/wav2vec2-conformer-rel-pos-large": W2V_CONFORMER_REL_LARGE,
    "facebook/wav2vec2-conformer-rel-pos-large-960h-ft": replace(W2V_CONFORMER_REL_LARGE, name="facebook/wav2vec2-conformer-rel-pos-large-960h-ft"),
}


def tiny_geometry(family: str, *, hidden: int = 128, heads: int = 2, layers: int = 2,
                  ffn: int = 256, conv_dim: int = 64, pos_groups: int = 2, text_conv_kernel: int = 0,
                  base: bool = False, conv_bias: bool = False, depthwise_kernel: int = 31, left_max: int = 64,
                  right_max: int = 8, position_type: str = "rotary") -> EncoderGeometry:
    """Small geometries with the real kernel/stride tuples; used by the parity
    fixtures under tests/golden.  ``hidden // heads`` selects
    the head-dim code path (64 WavLM/Whisper, 80 HuBERT-XL, 120 XLS-R-2B) and
    ``hidden // pos_groups`` the pos-conv group width (64 / 80 / 120 in the real models).  ``base=True``: the *-base form of a
    speech family (GroupNorm stem, post-LN encoder, no conv bias).  ``conv_bias``: data2vec-audio only (the other families fix it)."""
    if family == FAMILY_ROBERTA:
        return EncoderGeometry(family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn,
                               vocab_size=300, max_positions=90, name=f"tiny-{family}-d{hidden}h{heads}")
    if family == FAMILY_DEBERTA:
        # 16 buckets: relative distances beyond +-8 are log-bucketed already at 80 tokens, like +-128 at 512 in v3-large
        return EncoderGeometry(family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn, vocab_size=300,
                               max_positions=512, pad_token_id=0, type_vocab_size=0, layer_norm_eps=1e-7,
                               position_buckets=16, text_conv_kernel=text_conv_kernel,
                               name=f"tiny-{family}-d{hidden}h{heads}" + ("-conv" if text_conv_kernel else ""))
    if family == FAMILY_WHISPER:
        return EncoderGeometry(family=family, num_layers=layers, hidden=hidden, heads=heads,
                               ffn=ffn, n_mels=128, max_source_positions=1500,
                               name=f"tiny-{family}-d{hidden}h{heads}")
    if family == FAMILY_W2V_BERT:
        return EncoderGeometry(family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn, conv_depthwise_kernel=depthwise_kernel,
                               left_max_positions=left_max, right_max_positions=right_max,
                               name=f"tiny-w2v-bert-d{hidden}h{heads}")
    if family == FAMILY_W2V_CONFORMER:
        return EncoderGeometry(family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn, conv_dim=(conv_dim,) * 7,
                               conv_bias=conv_bias, conv_depthwise_kernel=depthwise_kernel, position_type=position_type,
                               max_source_positions=5000, name=f"tiny-w2v-conformer-{position_type}-d{hidden}h{heads}")
    if family == FAMILY_DATA2VEC_AUDIO:
        return EncoderGeometry(
            family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn, conv_dim=(conv_dim,) * 7, conv_bias=conv_bias,
            stable_layer_norm=False, pos_conv_kernel=19, pos_conv_groups=pos_groups, pos_conv_layers=5, pos_conv_norm="layer",
            name=f"tiny-{family}-d{hidden}h{heads}g{pos_groups}")
    if base:
        return EncoderGeometry(
            family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn,
            conv_dim=(conv_dim,) * 7, conv_bias=False, pos_conv_groups=pos_groups,
            feat_extract_norm="group", stable_layer_norm=False,
            name=f"tiny-{family}-base-d{hidden}h{heads}")
    return EncoderGeometry(
        family=family, num_layers=layers, hidden=hidden, heads=heads, ffn=ffn,
        conv_dim=(conv_dim,) * 7, conv_bias=(family != FAMILY_WAVLM),
        pos_conv_groups=pos_groups,
        name=f"tiny-{family}-d{hidden}h{heads}")


def geometry_for(ssl_type: str) -> EncoderGeometry:
    """Map ``--ssl_type`` to a geometry.  Unknown names raise ``OSError`` because
    that is what ``from_pretrained`` raises in the reference and what its driver
    catches (preprocess_speech.py:115-117)."""
    key = ssl_type.strip()
    if key in _REGISTRY:
        return _REGISTRY[key]
    low = key.lower()
    for name, geo in _REGISTRY.items():
        if low == name.lower() or low == name.split("/")[-1].lower():
            return geo
    raise OSError(f"No geometry registered for ssl_type '{ssl_type}'")


def geometry_from_config(cfg: dict, name: str = "") -> EncoderGeometry:
    """Geometry from a checkpoint's ``config.json`` -- what ``AutoModel.from_pretrained(--ssl_type)`` reads for ANY hub id or
    local snapshot (preprocess_speech.py:111-112, preprocess_whisper.py:119-120), so fine-tunes published under another name
    work without a registry entry.  Two speech forms are implemented: the layer-norm stem with a stable-LayerNorm encoder
    (*-large / xlarge / XLS-R) and the GroupNorm stem with a post-LayerNorm encoder (*-base: ``feat_extract_norm="group"``,
    ``do_stable_layer_norm=False``).  For these three model types the two mixed combinations, which none of their published
    checkpoints uses, are refused with ``OSError``, the class the reference's driver reports as "No pretrained model found"
    (:115-117).  data2vec-audio always pairs the layer-norm stem with a post-LayerNorm encoder."""
    mt = str(cfg.get("model_type", "")).lower()
    name = name or str(cfg.get("_name_or_path", "")) or mt
    if mt in (FAMILY_WAVLM, FAMILY_WAV2VEC2, FAMILY_HUBERT):
        norm, stable = cfg.get("feat_extract_norm", "group"), bool(cfg.get("do_stable_layer_norm", False))
        if norm not in ("layer", "group"):
            raise OSError(f"{name}: feat_extract_norm='{norm}' is not supported")
        if norm != "layer" and stable:
            raise OSError(f"{name}: feat_extract_norm='{cfg.get('feat_extract_norm', 'group')}' (GroupNorm over time) is not supported; "
                          "the path implements the layer-norm feature extractor of the *-large / xlarge / XLS-R checkpoints")
        if norm == "layer" and not stable:
            raise OSError(f"{name}: do_stable_layer_norm=False (post-LayerNorm encoder) is not supported")
        if mt == FAMILY_HUBERT and not cfg.get("feat_proj_layer_norm", True):
            raise OSError(f"{name}: feat_proj_layer_norm=False is not supported")
        conv_dim = tuple(int(c) for c in cfg.get("conv_dim", (512,) * 7))
        return EncoderGeometry(
            family=mt, num_layers=int(cfg["num_hidden_layers"]), hidden=int(cfg["hidden_size"]),
            heads=int(cfg["num_attention_heads"]), ffn=int(cfg["intermediate_size"]), conv_dim=conv_dim,
            conv_kernel=tuple(int(k) for k in cfg.get("conv_kernel", (10, 3, 3, 3, 3, 2, 2))),
            conv_stride=tuple(int(k) for k in cfg.get("conv_stride", (5, 2, 2, 2, 2, 2, 2))),
            conv_bias=bool(cfg.get("conv_bias", False)), feat_proj_layer_norm=bool(cfg.get("feat_proj_layer_norm", True)),
            pos_conv_kernel=int(cfg.get("num_conv_pos_embeddings", 128)), pos_conv_groups=int(cfg.get("num_conv_pos_embedding_groups", 16)),
            num_buckets=int(cfg.get("num_buckets", 320)), max_bucket_distance=int(cfg.get("max_bucket_distance", 800)),
            layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)), feat_extract_norm=norm, stable_layer_norm=stable, name=name)
    if mt == FAMILY_WHISPER:
        geo = EncoderGeometry(
            family=FAMILY_WHISPER, num_layers=int(cfg["encoder_layers"]), hidden=int(cfg["d_model"]),
            heads=int(cfg["encoder_attention_heads"]), ffn=int(cfg["encoder_ffn_dim"]), n_mels=int(cfg.get("num_mel_bins", 80)),
            max_source_positions=int(cfg.get("max_source_positions", 1500)), name=name)
        if int(cfg.get("decoder_layers", 0)) > 0 and "vocab_size" in cfg:
            geo = with_decoder(geo, cfg["decoder_layers"], cfg.get("decoder_attention_heads", cfg["encoder_attention_heads"]),
                               cfg.get("decoder_ffn_dim", cfg["encoder_ffn_dim"]), cfg["vocab_size"], cfg.get("max_target_positions", 448))
        return geo
    if mt in ("roberta", "xlm-roberta"):
        return EncoderGeometry(
            family=FAMILY_ROBERTA, num_layers=int(cfg["num_hidden_layers"]), hidden=int(cfg["hidden_size"]),
            heads=int(cfg["num_attention_heads"]), ffn=int(cfg["intermediate_size"]), vocab_size=int(cfg["vocab_size"]),
            max_positions=int(cfg.get("max_position_embeddings", 514)), pad_token_id=int(cfg.get("pad_token_id", 1)),
            type_vocab_size=int(cfg.get("type_vocab_size", 1)), layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)), name=name)
    if mt == "deberta-v2":
        pos_att = cfg.get("pos_att_type") or []
        pos_att = pos_att.split("|") if isinstance(pos_att, str) else list(pos_att)
        if not cfg.get("relative_attention", False) or sorted(pos_att) != ["c2p", "p2c"] or not cfg.get("share_att_key", False) \
                or cfg.get("position_biased_input", True) or str(cfg.get("norm_rel_ebd", "none")) != "layer_norm":
            raise OSError(f"{name}: only the deberta-v3 / v2-xlarge attention configuration is supported (relative_attention, "
                          "pos_att_type p2c|c2p, share_att_key, norm_rel_ebd layer_norm, no absolute positions)")
        return EncoderGeometry(
            family=FAMILY_DEBERTA, num_layers=int(cfg["num_hidden_layers"]), hidden=int(cfg["hidden_size"]),
            heads=int(cfg["num_attention_heads"]), ffn=int(cfg["intermediate_size"]), vocab_size=int(cfg["vocab_size"]),
            max_positions=int(cfg.get("max_position_embeddings", 512)), pad_token_id=int(cfg.get("pad_token_id", 0)),
            type_vocab_size=int(cfg.get("type_vocab_size", 0)), layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-7)),
            position_buckets=int(cfg.get("position_buckets", 256)), text_conv_kernel=int(cfg.get("conv_kernel_size", 0) or 0), name=name)
    if mt == FAMILY_DATA2VEC_AUDIO:
        # HF Data2VecAudioConfig: the positional kernel is conv_pos_kernel_size and num_conv_pos_embeddings is the number of conv
        # LAYERS (in the wavlm / wav2vec2 / hubert configs that key is the kernel).  The stem is always the layer-norm one
        # (Data2VecAudioConvLayer) and the encoder always post-LN (Data2VecAudioEncoder); the config has no key for either.
        if cfg.get("add_adapter", False):
            raise OSError(f"{name}: add_adapter=True (an adapter stack after the encoder) is not supported")
        k = int(cfg.get("conv_pos_kernel_size", 19))
        if k % 2 == 0:
            raise OSError(f"{name}: an even conv_pos_kernel_size ({k}) is not supported (Data2VecAudioPadLayer drops the last frame)")
        return EncoderGeometry(
            family=FAMILY_DATA2VEC_AUDIO, num_layers=int(cfg["num_hidden_layers"]), hidden=int(cfg["hidden_size"]),
            heads=int(cfg["num_attention_heads"]), ffn=int(cfg["intermediate_size"]),
            conv_dim=tuple(int(c) for c in cfg.get("conv_dim", (512,) * 7)),
            conv_kernel=tuple(int(c) for c in cfg.get("conv_kernel", (10, 3, 3, 3, 3, 2, 2))),
            conv_stride=tuple(int(c) for c in cfg.get("conv_stride", (5, 2, 2, 2, 2, 2, 2))),
            conv_bias=bool(cfg.get("conv_bias", False)), feat_extract_norm="layer", stable_layer_norm=False,
            pos_conv_kernel=k, pos_conv_groups=int(cfg.get("num_conv_pos_embedding_groups", 16)),
            pos_conv_layers=int(cfg.get("num_conv_pos_embeddings", 5)), pos_conv_norm="layer",
            layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)), name=name)
    if mt == FAMILY_W2V_BERT:
        # HF Wav2Vec2BertConfig.  Built: relative-key positions, the swish activation, no adapter (facebook/w2v-bert-2.0's settings).
        pos = cfg.get("position_embeddings_type", "relative_key")
        if pos != "relative_key":
            raise OSError(f"{name}: position_embeddings_type='{pos}' is not supported (the path implements relative_key)")
        if cfg.get("add_adapter", False):
            raise OSError(f"{name}: add_adapter=True (an adapter stack after the encoder) is not supported")
        if str(cfg.get("hidden_act", "swish")) not in ("swish", "silu"):
            raise OSError(f"{name}: hidden_act='{cfg.get('hidden_act')}' is not supported (the path implements swish)")
        k = int(cfg.get("conv_depthwise_kernel_size", 31))
        if k % 2 == 0:
            raise OSError(f"{name}: an even conv_depthwise_kernel_size ({k}) is not supported")
        if k > 31:
            raise OSError(f"{name}: conv_depthwise_kernel_size {k} is beyond the 31 taps the convolution-module kernel holds")
        lm, rm = int(cfg.get("left_max_position_embeddings", 64)), int(cfg.get("right_max_position_embeddings", 8))
        if lm < 0 or rm < 0 or lm + rm + 1 > 128:
            raise OSError(f"{name}: left_max_position_embeddings + right_max_position_embeddings + 1 = {lm + rm + 1} is beyond 128 distances")
        fdim, stride = int(cfg.get("feature_projection_input_dim", 160)), int(cfg.get("fbank_stride", 2))
        if stride < 1 or fdim % stride:
            raise OSError(f"{name}: feature_projection_input_dim {fdim} is not a multiple of the frame stacking {stride}")
        return EncoderGeometry(
            family=FAMILY_W2V_BERT, num_layers=int(cfg["num_hidden_layers"]), hidden=int(cfg["hidden_size"]),
            heads=int(cfg["num_attention_heads"]), ffn=int(cfg["intermediate_size"]), fbank_mels=fdim // stride, fbank_stride=stride,
            conv_depthwise_kernel=k, left_max_positions=lm, right_max_positions=rm,
            layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)), name=name)
    if mt == FAMILY_W2V_CONFORMER:
        # HF Wav2Vec2ConformerConfig.  Built: the layer-norm stem, rotary or relative positions, swish, no adapter (the settings of
        # facebook/wav2vec2-conformer-{rope,rel-pos}-large and their -960h-ft fine-tunes).  The class defaults are NOT those settings
        # (feat_extract_norm "group", hidden_act "gelu"), so a missing key is refused like the value it stands for.
        if cfg.get("add_adapter", False):
            raise OSError(f"{name}: add_adapter=True (an adapter stack after the encoder) is not supported")
        norm = cfg.get("feat_extract_norm", "group")
        if norm != "layer":
            raise OSError(f"{name}: feat_extract_norm='{norm}' is not supported (the path implements the layer-norm feature extractor "
                          "of the published wav2vec2-conformer checkpoints)")
        act = str(cfg.get("hidden_act", "gelu"))
        if act not in ("swish", "silu"):
            raise OSError(f"{name}: hidden_act='{act}' is not supported (the path implements swish)")
        k = int(cfg.get("conv_depthwise_kernel_size", 31))
        if k % 2 == 0:
            raise OSError(f"{name}: an even conv_depthwise_kernel_size ({k}) is not supported")
        if k > 31:
            raise OSError(f"{name}: conv_depthwise_kernel_size {k} is beyond the 31 taps the convolution-module kernel holds")
        hidden, heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        if heads < 1 or hidden % heads or hidden // heads != 64:
            raise OSError(f"{name}: hidden_size {hidden} / num_attention_heads {heads} is not a head dim of 64, the one the conformer "
                          "attention is built for")
        pos = cfg.get("position_embeddings_type", "relative")
        if pos not in W2V_CONFORMER_POSITION_TYPES:
            raise OSError(f"{name}: position_embeddings_type='{pos}' is not supported (the path implements "
                          + " / ".join(W2V_CONFORMER_POSITION_TYPES) + ")")
        return EncoderGeometry(
            family=FAMILY_W2V_CONFORMER, num_layers=int(cfg["num_hidden_layers"]), hidden=hidden, heads=heads,
            ffn=int(cfg["intermediate_size"]), conv_dim=tuple(int(c) for c in cfg.get("conv_dim", (512,) * 7)),
            conv_kernel=tuple(int(c) for c in cfg.get("conv_kernel", (10, 3, 3, 3, 3, 2, 2))),
            conv_stride=tuple(int(c) for c in cfg.get("conv_stride", (5, 2, 2, 2, 2, 2, 2))),
            conv_bias=bool(cfg.get("conv_bias", False)), feat_extract_norm="layer", conv_depthwise_kernel=k, position_type=pos,
            rotary_base=int(cfg.get("rotary_embedding_base", 10000)), max_source_positions=int(cfg.get("max_source_positions", 5000)),
            layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)), name=name)
    raise OSError(f"{name}: model_type '{mt}' is not an encoder this path implements "
                  "(wavlm / wav2vec2 / hubert / data2vec-audio / wav2vec2-bert / wav2vec2-conformer / whisper / roberta / deberta-v2)")


def find_config_json(ssl_type: str, checkpoint: str = "") -> str:
    """Path of the ``config.json`` that belongs to the weights the driver will load: next to ``--checkpoint`` (a snapshot
    directory or a file inside one), else in the offline HF cache snapshot of ``--ssl_type``; "" when there is none."""
    import os
    cands = []
    if checkpoint:
        cands.append(os.path.join(checkpoint if os.path.isdir(checkpoint) else os.path.dirname(os.path.abspath(checkpoint)), "config.json"))
    elif os.path.isdir(ssl_type):
        cands.append(os.path.join(ssl_type, "config.json"))
    home = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
    snap = os.path.join(home, "hub", "models--" + ssl_type.replace("/", "--"), "snapshots")
    if not checkpoint and os.path.isdir(snap):
        cands += [os.path.join(snap, rev, "config.json") for rev in sorted(os.listdir(snap))]
    for c in cands:
        if os.path.isfile(c):
            return c
    return ""


def resolve_geometry(ssl_type: str, checkpoint: str = "") -> EncoderGeometry:
    """``config.json`` of the checkpoint when there is one (any name), else the built-in table by ``--ssl_type``."""
    import json
    path = find_config_json(ssl_type, checkpoint)
    if path:
        try:
            with open(path, "r") as f:
                cfg = json.load(f)
        except (OSError, ValueError) as e:
            raise OSError(f"cannot read {path}: {e}")
        return geometry_from_config(cfg, name=ssl_type)
    return geometry_for(ssl_type)


def find_preprocessor_config(ssl_type: str, checkpoint: str = "") -> str:
    """Path of the ``preprocessor_config.json`` beside the ``config.json`` that ``find_config_json`` picks ("" when there is none):
    what ``AutoFeatureExtractor.from_pretrained(--ssl_type)`` reads (preprocess_speech.py:43)."""
    import os
    cfg = find_config_json(ssl_type, checkpoint)
    if cfg:
        p = os.path.join(os.path.dirname(cfg), "preprocessor_config.json")
        return p if os.path.isfile(p) else ""
    return ""


def resolve_do_normalize(ssl_type: str, checkpoint: str = "") -> bool:
    """``do_normalize`` of the checkpoint's feature extractor: the zero-mean / unit-variance input normalisation
    (HF feature_extraction_wav2vec2.py).  True when the snapshot has no ``preprocessor_config.json`` (the path's behaviour
    before it read the file; also the value of the *-large checkpoints)."""
    import json
    path = find_preprocessor_config(ssl_type, checkpoint)
    if not path:
        return True
    try:
        with open(path, "r") as f:
            cfg = json.load(f)
    except (OSError, ValueError) as e:
        raise OSError(f"cannot read {path}: {e}")
    return bool(cfg.get("do_normalize", True))


def resolve_fbank(geo: EncoderGeometry, ssl_type: str, checkpoint: str = "") -> EncoderGeometry:
    """A w2v-BERT geometry with the front end's mel count and frame stacking taken from the snapshot's ``preprocessor_config.json``
    (HF SeamlessM4TFeatureExtractor: ``num_mel_bins`` / ``feature_size`` and ``stride``); 80 and 2 when there is no such file.  Their
    product must be the model's ``feature_projection_input_dim``."""
    import json
    if geo.family != FAMILY_W2V_BERT:
        return geo
    path = find_preprocessor_config(ssl_type, checkpoint)
    mels, stride = 80, 2
    if path:
        try:
            with open(path, "r") as f:
                cfg = json.load(f)
        except (OSError, ValueError) as e:
            raise OSError(f"cannot read {path}: {e}")
        mels, stride = int(cfg.get("num_mel_bins", cfg.get("feature_size", 80))), int(cfg.get("stride", 2))
    if mels * stride != geo.fbank_dim:
        raise OSError(f"{ssl_type}: the feature extractor stacks {stride} frames of {mels} mel bins, the model's feature projection "
                      f"reads {geo.fbank_dim} columns")
    return replace(geo, fbank_mels=mels, fbank_stride=stride)


def with_layers(geo: EncoderGeometry, layers: int) -> EncoderGeometry:
    g = replace(geo, num_layers=layers)
    if geo.decoder is not None:                             # replace() goes through __init__, which knows no decoder
        object.__setattr__(g, "_decoder", geo.decoder)
    return g


# The four fixture geometries under tests/golden (head dims 64 / 120 / 80 / 64 and
# pos-conv group widths 64 / 120 / 80, i.e. every code path of the real models).
TINY_WAVLM = tiny_geometry(FAMILY_WAVLM, hidden=128, heads=2, ffn=256, pos_groups=2)
TINY_WAV2VEC2 = tiny_geometry(FAMILY_WAV2VEC2, hidden=960, heads=8, ffn=512, pos_groups=8)
TINY_HUBERT = tiny_geometry(FAMILY_HUBERT, hidden=320, heads=4, ffn=384, pos_groups=4)
TINY_WHISPER = tiny_geometry(FAMILY_WHISPER, hidden=128, heads=2, ffn=256)
# ... with the decoder of tests/golden/tiny_whisper_dec_d128h2.npz: 522 = 51 866 mod 8 (+ 8 k), so the vocabulary padding is live
TINY_WHISPER_DEC = with_decoder(replace(TINY_WHISPER, name="tiny-whisper-dec-d128h2"), 2, 2, 512, 522, 64)
TINY_ROBERTA = tiny_geometry(FAMILY_ROBERTA, hidden=128, heads=2, ffn=256)
TINY_DEBERTA = tiny_geometry(FAMILY_DEBERTA, hidden=128, heads=2, ffn=256)
TINY_DEBERTA_CONV = tiny_geometry(FAMILY_DEBERTA, hidden=128, heads=2, ffn=256, text_conv_kernel=3)      # deberta-v2-xlarge style
# *-base fixture geometries (GroupNorm stem, post-LN encoder; tests/golden/tiny_*_base_*.npz)
TINY_WAVLM_BASE = tiny_geometry(FAMILY_WAVLM, hidden=128, heads=2, ffn=256, pos_groups=2, base=True)
TINY_WAV2VEC2_BASE = tiny_geometry(FAMILY_WAV2VEC2, hidden=128, heads=2, ffn=256, pos_groups=2, base=True)
TINY_HUBERT_BASE = tiny_geometry(FAMILY_HUBERT, hidden=128, heads=2, ffn=256, pos_groups=2, base=True)
# data2vec-audio fixture geometries (tests/golden/tiny_data2vec_audio_*.npz): positional group width 64, and 48 -- the real base
# model's (768 / 16), not a multiple of 64, so the stack's GEMMs read the padded channels of pos_kc
TINY_DATA2VEC_AUDIO = tiny_geometry(FAMILY_DATA2VEC_AUDIO, hidden=128, heads=2, ffn=256, pos_groups=2)
TINY_DATA2VEC_AUDIO_G48 = tiny_geometry(FAMILY_DATA2VEC_AUDIO, hidden=192, heads=3, ffn=256, pos_groups=4, conv_bias=True)
# w2v-BERT fixture geometries (tests/golden/tiny_w2v_bert_*.npz): the checkpoint's kernel and clamp, and a second set (7 taps, clamp -5 .. 3,
# three heads) that no constant of the first survives
TINY_W2V_BERT = tiny_geometry(FAMILY_W2V_BERT, hidden=128, heads=2, ffn=256)
TINY_W2V_BERT_H3 = tiny_geometry(FAMILY_W2V_BERT, hidden=192, heads=3, ffn=384, depthwise_kernel=7, left_max=5, right_max=3)
# wav2vec2-conformer fixture geometries (tests/golden/tiny_w2v_conformer_*.npz): one per position type, two and three heads of 64
TINY_W2V_CONFORMER_ROPE = tiny_geometry(FAMILY_W2V_CONFORMER, hidden=128, heads=2, ffn=256, conv_bias=True, position_type="rotary")
TINY_W2V_CONFORMER_REL = tiny_geometry(FAMILY_W2V_CONFORMER, hidden=192, heads=3, ffn=384, conv_bias=True, position_type="relative")


@dataclass(frozen=True)
class GenerationSpec:
    """What the short-form path of HF's ``WhisperGenerationMixin.generate`` reads from ``generation_config.json`` when it is called with
    defaults (greedy, no timestamps): prompt ``[start, language, task, no_timestamps]``, ``suppress_tokens`` at every generated
    position, ``begin_suppress_tokens`` at the first one too.  ``language`` None: detected per utterance (one step on ``[start]``,
    logits restricted to ``lang_ids``, argmax)."""
    decoder_start_token_id: int
    eos_token_id: int
    pad_token_id: int
    suppress_tokens: Tuple[int, ...]
    begin_suppress_tokens: Tuple[int, ...]
    no_timestamps_token_id: int
    lang_ids: Tuple[int, ...]
    task_id: int
    max_length: int = 448
    language: object = None            # None, a token id, or a key of ``lang_to_id`` ("en" / "<|en|>") resolved by from_snapshot
    alignment_heads: Tuple[Tuple[int, int], ...] = ()   # (decoder layer, head) pairs whose cross-attention carries the token times; () = absent
    median_filter_width: int = 7       # config.json's (not generation_config.json's): the transcriber fills it in
    num_beams: int = 1                 # 1: greedy; 2..8: HF's beam search with early_stopping = False (engine.WhisperDecoder.generate)
    length_penalty: float = 1.0        # the exponent of the generated length a finished beam's score is divided by
    max_initial_timestamp_index: Optional[int] = None   # None when absent, as HF's WhisperTimeStampLogitsProcessor reads it
    no_speech_token_id: Optional[int] = None            # None: HF's own choice, no_timestamps_token_id - 1 (``no_speech_token``)
    logprob_threshold: Optional[float] = None           # HF generate()'s three thresholds; None: not set (transcribe.need_fallback)
    no_speech_threshold: Optional[float] = None
    compression_ratio_threshold: Optional[float] = None

    PROMPT_LEN = 4
    MAX_BEAMS = 8
    TIME_PRECISION = 0.02              # seconds per encoder frame

    def prompt_len(self, timestamps: bool = False) -> int:
        """The prompt length of a run: ``PROMPT_LEN`` with ``<|notimestamps|>``, one less for a segment-timestamps run, whose prompt is
        ``[start, language, task]``."""
        return self.PROMPT_LEN - 1 if timestamps else self.PROMPT_LEN

    @property
    def timestamp_begin(self) -> int:
        """The id of ``<|0.00|>``: every id from here on is a timestamp token (HF: ``no_timestamps_token_id + 1``)."""
        return self.no_timestamps_token_id + 1

    @property
    def no_speech_token(self) -> int:
        """The id whose probability at the first decoder position is the no-speech probability (HF: ``no_timestamps_token_id - 1``)."""
        return self.no_timestamps_token_id - 1 if self.no_speech_token_id is None else int(self.no_speech_token_id)

    @property
    def thresholds(self) -> dict:
        """The three thresholds by HF's names, None where not set."""
        return dict(logprob_threshold=self.logprob_threshold, no_speech_threshold=self.no_speech_threshold,
                    compression_ratio_threshold=self.compression_ratio_threshold)

    def require_alignment_heads(self) -> Tuple[Tuple[int, int], ...]:
        """The alignment heads, or the error that names what is missing: token times were asked of a checkpoint that has none."""
        if not self.alignment_heads:
            raise ValueError("token times need `alignment_heads` in generation_config.json, and this checkpoint's has none")
        return self.alignment_heads

    @staticmethod
    def from_config(cfg: dict, language=None) -> "GenerationSpec":
        lang_to_id = {str(k): int(v) for k, v in (cfg.get("lang_to_id") or {}).items()}
        task_to_id = cfg.get("task_to_id") or {}
        missing = [k for k in ("decoder_start_token_id", "eos_token_id", "no_timestamps_token_id") if cfg.get(k) is None]
        if missing or not lang_to_id or "transcribe" not in task_to_id:
            raise OSError("generation_config.json lacks " + ", ".join(missing + ["lang_to_id"] * (not lang_to_id)
                                                                      + ["task_to_id.transcribe"] * ("transcribe" not in task_to_id)))
        if language is not None and not isinstance(language, int):
            key = str(language)
            for cand in (key, f"<|{key}|>"):
                if cand in lang_to_id:
                    language = lang_to_id[cand]
                    break
            else:
                raise ValueError(f"language '{key}' is not in the checkpoint's lang_to_id")
        eos = cfg["eos_token_id"]
        eos = int(eos[0] if isinstance(eos, (list, tuple)) else eos)
        pad = cfg.get("pad_token_id")
        heads = cfg.get("alignment_heads") or ()
        if any(not isinstance(h, (list, tuple)) or len(h) != 2 or int(h[0]) < 0 or int(h[1]) < 0 for h in heads):
            raise OSError("generation_config.json: alignment_heads must be a list of [layer, head] pairs")
        early = cfg.get("early_stopping")
        if early not in (None, False):
            raise OSError(f"generation_config.json: early_stopping={early!r} is not built (beam search runs HF's early_stopping=false only)")
        beams = cfg.get("num_beams")
        beams = 1 if beams is None else beams
        if isinstance(beams, bool) or not isinstance(beams, int) or not 1 <= beams <= GenerationSpec.MAX_BEAMS:
            raise OSError(f"generation_config.json: num_beams={beams!r} (1..{GenerationSpec.MAX_BEAMS})")
        initial = cfg.get("max_initial_timestamp_index")
        if initial is not None and (isinstance(initial, bool) or not isinstance(initial, int) or initial < 0):
            raise OSError(f"generation_config.json: max_initial_timestamp_index={initial!r} (a non-negative integer, or absent)")
        penalty = cfg.get("length_penalty")
        penalty = 1.0 if penalty is None else penalty
        if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or penalty != penalty or abs(penalty) == float("inf"):
            raise OSError(f"generation_config.json: length_penalty={penalty!r} (a finite number)")
        limits = {}
        for k in ("logprob_threshold", "no_speech_threshold", "compression_ratio_threshold"):
            v = cfg.get(k)
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf")):
                raise OSError(f"generation_config.json: {k}={v!r} (a finite number, or absent)")
            limits[k] = None if v is None else float(v)
        ns = cfg.get("no_speech_token_id")
        if ns is not None and (isinstance(ns, bool) or not isinstance(ns, int) or ns < 0):
            raise OSError(f"generation_config.json: no_speech_token_id={ns!r} (a token id, or absent)")
        return GenerationSpec(
            no_speech_token_id=ns, **limits,
            num_beams=beams, length_penalty=float(penalty), max_initial_timestamp_index=initial,
            decoder_start_token_id=int(cfg["decoder_start_token_id"]), eos_token_id=eos, pad_token_id=eos if pad is None else int(pad),
            suppress_tokens=tuple(int(t) for t in cfg.get("suppress_tokens") or ()),
            begin_suppress_tokens=tuple(int(t) for t in cfg.get("begin_suppress_tokens") or ()),
            no_timestamps_token_id=int(cfg["no_timestamps_token_id"]), lang_ids=tuple(sorted(lang_to_id.values())),
            task_id=int(task_to_id["transcribe"]), max_length=int(cfg.get("max_length", 448)), language=language,
            alignment_heads=tuple((int(l), int(h)) for l, h in heads), median_filter_width=int(cfg.get("median_filter_width", 7)))

    @staticmethod
    def from_snapshot(directory: str, language=None) -> "GenerationSpec":
        """``generation_config.json`` of a local snapshot directory (or of the directory a checkpoint file lies in)."""
        import json
        import os
        d = directory if os.path.isdir(directory) else os.path.dirname(os.path.abspath(directory))
        path = os.path.join(d, "generation_config.json")
        try:
            with open(path, "r") as f:
                cfg = json.load(f)
        except (OSError, ValueError) as e:
            raise OSError(f"cannot read {path}: {e}")
        return GenerationSpec.from_config(cfg, language)


# The seven hub classes that share one head (HF *ForSequenceClassification of the speech families, WhisperForAudioClassification):
# optional softmax-weighted sum of the hidden states -> projector -> mean over the frames -> classifier (engine.ClassifierHead).
AUDIO_CLASSIFICATION_ARCHITECTURES = (
    "Wav2Vec2ForSequenceClassification", "WavLMForSequenceClassification", "HubertForSequenceClassification",
    "Data2VecAudioForSequenceClassification", "Wav2Vec2BertForSequenceClassification", "WhisperForAudioClassification",
    "Wav2Vec2ConformerForSequenceClassification")


@dataclass(frozen=True)
class ClassifierSpec:
    """What ``AutoModelForAudioClassification`` reads from ``config.json`` for that head.  ``labels``: ``id2label`` in index order
    (``LABEL_i`` where the config has none, as ``PretrainedConfig`` names them)."""
    use_weighted_layer_sum: bool
    classifier_proj_size: int
    num_labels: int
    labels: Tuple[str, ...]
    architecture: str = ""

    @staticmethod
    def from_config(cfg: dict, name: str = "") -> Optional["ClassifierSpec"]:
        """The spec of a snapshot whose ``architectures[0]`` is one of the six classes, else None (such a snapshot runs as a bare
        encoder, as before)."""
        arch = cfg.get("architectures") or []
        arch = arch[0] if isinstance(arch, (list, tuple)) and arch else (arch if isinstance(arch, str) else "")
        if arch not in AUDIO_CLASSIFICATION_ARCHITECTURES:
            return None
        name = name or str(cfg.get("_name_or_path", "")) or arch
        if cfg.get("add_adapter", False):
            # HF: "Sequence classification does not support the use of <model> adapters (config.add_adapter=True)"
            raise OSError(f"{name}: {arch} does not support adapters (add_adapter=True)")
        id2label = cfg.get("id2label")
        if id2label:
            by_index = {int(k): str(v) for k, v in id2label.items()}
            n = len(by_index)
            if sorted(by_index) != list(range(n)):
                raise OSError(f"{name}: id2label does not number its labels 0..{n - 1}")
            labels = tuple(by_index[i] for i in range(n))
        else:
            n = int(cfg.get("num_labels", 2))
            labels = tuple(f"LABEL_{i}" for i in range(n))
        if n < 1:
            raise OSError(f"{name}: no labels")
        return ClassifierSpec(use_weighted_layer_sum=bool(cfg.get("use_weighted_layer_sum", False)),
                              classifier_proj_size=int(cfg.get("classifier_proj_size", 256)), num_labels=n, labels=labels, architecture=arch)


def resolve_classifier(ssl_type: str, checkpoint: str = "") -> Optional[ClassifierSpec]:
    """``ClassifierSpec`` of the ``config.json`` that ``find_config_json`` picks; None when there is no such file or it names another class."""
    import json
    path = find_config_json(ssl_type, checkpoint)
    if not path:
        return None
    try:
        with open(path, "r") as f:
            cfg = json.load(f)
    except (OSError, ValueError) as e:
        raise OSError(f"cannot read {path}: {e}")
    return ClassifierSpec.from_config(cfg, name=ssl_type)


# The hub classes that share the x-vector head (HF *ForXVector, what ``AutoModelForAudioXVector`` loads): optional softmax-weighted sum of
# the hidden states -> projector -> ReLU TDNN layers -> statistics pooling -> feature_extractor -> classifier (engine.XVectorHead).
XVECTOR_ARCHITECTURES = ("Wav2Vec2ForXVector", "WavLMForXVector", "Data2VecAudioForXVector", "Wav2Vec2BertForXVector")
# ... and the two it does not run behind: UniSpeech-SAT's encoder is not built, the conformer encoders' x-vector head is not wired
XVECTOR_UNBUILT_ARCHITECTURES = ("UniSpeechSatForXVector", "Wav2Vec2ConformerForXVector")


@dataclass(frozen=True)
class TdnnLayout:
    """Where the rows of a ragged batch lie at every level of a TDNN stack: ``offs[0]`` the [B + 1] input frame offsets, ``offs[i]`` those
    of layer i's packed output rows (T_i = T_{i-1} - d_i (k_i - 1) per utterance)."""
    offs: Tuple[Tuple[int, ...], ...]
    kernel: Tuple[int, ...]
    dilation: Tuple[int, ...]

    def first_rows(self, i: int):
        """numpy int64 [rows of layer i]: the input row (in layer i - 1's packed rows) under tap 0 of every output row of layer i
        (1 <= i <= len(kernel)); tap j reads ``dilation[i - 1] * j`` rows further.  What ser_ragged_index builds on the device."""
        import numpy as np
        src, dst = self.offs[i - 1], self.offs[i]
        return np.concatenate([src[b] + np.arange(dst[b + 1] - dst[b], dtype=np.int64) for b in range(len(dst) - 1)]
                              + [np.zeros(0, dtype=np.int64)])


@dataclass(frozen=True)
class XVectorSpec:
    """What ``AutoModelForAudioXVector`` reads from ``config.json`` for that head."""
    tdnn_dim: Tuple[int, ...]
    tdnn_kernel: Tuple[int, ...]
    tdnn_dilation: Tuple[int, ...]
    xvector_output_dim: int
    use_weighted_layer_sum: bool
    num_labels: int = 2                # sizes ``objective.weight`` (training) only: HF's classifier is Linear(xvector_output_dim, xvector_output_dim)
    architecture: str = ""

    @property
    def context(self) -> int:
        """frames the TDNN stack consumes: T' = T - context"""
        return sum(d * (k - 1) for k, d in zip(self.tdnn_kernel, self.tdnn_dilation))

    @property
    def min_frames(self) -> int:
        """fewest encoder frames with T' >= 2, what the unbiased std needs"""
        return self.context + 2

    @staticmethod
    def from_config(cfg: dict, name: str = "") -> Optional["XVectorSpec"]:
        """The spec of a snapshot whose ``architectures[0]`` is one of ``XVECTOR_ARCHITECTURES``, else None.  ``OSError``: an x-vector
        class over an encoder that is not built, ``add_adapter``, TDNN lists of unequal length."""
        arch = cfg.get("architectures") or []
        arch = arch[0] if isinstance(arch, (list, tuple)) and arch else (arch if isinstance(arch, str) else "")
        name = name or str(cfg.get("_name_or_path", "")) or arch
        if arch in XVECTOR_UNBUILT_ARCHITECTURES:
            raise OSError(f"{name}: {arch} is not supported (its encoder is not built; the x-vector head runs behind "
                          + ", ".join(XVECTOR_ARCHITECTURES) + ")")
        if arch not in XVECTOR_ARCHITECTURES:
            return None
        if cfg.get("add_adapter", False):
            raise OSError(f"{name}: {arch} with add_adapter=True (an adapter stack after the encoder) is not supported")
        dim = tuple(int(v) for v in cfg.get("tdnn_dim", (512, 512, 512, 512, 1500)))
        kernel = tuple(int(v) for v in cfg.get("tdnn_kernel", (5, 3, 3, 1, 1)))
        dilation = tuple(int(v) for v in cfg.get("tdnn_dilation", (1, 2, 3, 1, 1)))
        if not (len(dim) == len(kernel) == len(dilation)) or not dim:
            raise OSError(f"{name}: tdnn_dim, tdnn_kernel and tdnn_dilation have {len(dim)}, {len(kernel)} and {len(dilation)} entries "
                          "(one per TDNN layer each)")
        if min(dim) < 1 or min(kernel) < 1 or min(dilation) < 1:
            raise OSError(f"{name}: tdnn_dim {dim}, tdnn_kernel {kernel} and tdnn_dilation {dilation} must be positive")
        id2label = cfg.get("id2label")
        n = len(id2label) if id2label else int(cfg.get("num_labels", 2))
        return XVectorSpec(tdnn_dim=dim, tdnn_kernel=kernel, tdnn_dilation=dilation, xvector_output_dim=int(cfg.get("xvector_output_dim", 512)),
                           use_weighted_layer_sum=bool(cfg.get("use_weighted_layer_sum", False)), num_labels=n, architecture=arch)

    def layout(self, frame_offs) -> TdnnLayout:
        """The per-layer packed offsets of a batch whose utterance b owns encoder rows ``frame_offs[b] .. frame_offs[b + 1] - 1``.
        ``ValueError`` naming the first utterance (by index) that keeps fewer than two rows: it has no unbiased std."""
        offs = [tuple(int(o) for o in frame_offs)]
        frames = [offs[0][b + 1] - offs[0][b] for b in range(len(offs[0]) - 1)]
        for b, t in enumerate(frames):
            if t < self.min_frames:
                raise ValueError(f"utterance {b}: {t} encoder frames leave {max(t - self.context, 0)} TDNN output rows; the unbiased std of "
                                 f"the statistics pooling needs 2 (at least {self.min_frames} frames)")
        for k, d in zip(self.tdnn_kernel, self.tdnn_dilation):
            frames = [t - d * (k - 1) for t in frames]
            acc = [0]
            for t in frames:
                acc.append(acc[-1] + t)
            offs.append(tuple(acc))
        return TdnnLayout(offs=tuple(offs), kernel=self.tdnn_kernel, dilation=self.tdnn_dilation)


def resolve_xvector(ssl_type: str, checkpoint: str = "") -> Optional[XVectorSpec]:
    """``XVectorSpec`` of the ``config.json`` that ``find_config_json`` picks; None when there is no such file or it names another class."""
    import json
    path = find_config_json(ssl_type, checkpoint)
    if not path:
        return None
    try:
        with open(path, "r") as f:
            cfg = json.load(f)
    except (OSError, ValueError) as e:
        raise OSError(f"cannot read {path}: {e}")
    return XVectorSpec.from_config(cfg, name=ssl_type)


# The hub classes that put a CTC head on the encoders built here (HF *ForCTC, what ``AutoModelForCTC`` loads): dropout ->
# lm_head(last_hidden_state) -> argmax per frame -> equal neighbours merged, blanks dropped (engine.CTCHead).
CTC_ARCHITECTURES = ("Wav2Vec2ForCTC", "HubertForCTC", "WavLMForCTC", "Data2VecAudioForCTC", "Wav2Vec2BertForCTC")
# ... and those it does not run behind: encoders that are not built, and the conformer encoders, whose CTC head is not wired
CTC_UNBUILT_ARCHITECTURES = ("UniSpeechForCTC", "UniSpeechSatForCTC", "Wav2Vec2ConformerForCTC", "SEWForCTC", "SEWDForCTC")


@dataclass(frozen=True)
class CTCSpec:
    """What ``AutoModelForCTC`` reads from ``config.json`` for that head.  ``blank``: ``pad_token_id``, the id
    ``Wav2Vec2CTCTokenizer`` drops after grouping."""
    vocab_size: int
    blank: int
    architecture: str = ""

    @staticmethod
    def from_config(cfg: dict, name: str = "") -> Optional["CTCSpec"]:
        """The spec of a snapshot whose ``architectures[0]`` is one of ``CTC_ARCHITECTURES``, else None.  ``OSError`` naming the class: a
        CTC class over an encoder that is not built, ``add_adapter``, a missing ``vocab_size`` or ``pad_token_id``."""
        arch = cfg.get("architectures") or []
        arch = arch[0] if isinstance(arch, (list, tuple)) and arch else (arch if isinstance(arch, str) else "")
        name = name or str(cfg.get("_name_or_path", "")) or arch
        if arch in CTC_UNBUILT_ARCHITECTURES:
            raise OSError(f"{name}: {arch} is not supported (its encoder is not built; the CTC head runs behind " + ", ".join(CTC_ARCHITECTURES) + ")")
        if arch not in CTC_ARCHITECTURES:
            return None
        if cfg.get("add_adapter", False):
            raise OSError(f"{name}: {arch} with add_adapter=True (an adapter stack after the encoder) is not supported")
        if cfg.get("vocab_size") is None:
            # HF: "You are trying to instantiate <class> with a configuration that does not define the vocabulary size of the language model head"
            raise OSError(f"{name}: {arch} without vocab_size (the width of lm_head) in config.json")
        if cfg.get("pad_token_id") is None:
            raise OSError(f"{name}: {arch} without pad_token_id (the CTC blank) in config.json")
        V, blank = int(cfg["vocab_size"]), int(cfg["pad_token_id"])
        if V < 1 or not 0 <= blank < V:
            raise OSError(f"{name}: {arch} with vocab_size {V} and pad_token_id {blank} (the blank must be one of the vocabulary)")
        return CTCSpec(vocab_size=V, blank=blank, architecture=arch)


def resolve_ctc(ssl_type: str, checkpoint: str = "") -> Optional[CTCSpec]:
    """``CTCSpec`` of the ``config.json`` that ``find_config_json`` picks; None when there is no such file or it names another class."""
    import json
    path = find_config_json(ssl_type, checkpoint)
    if not path:
        return None
    try:
        with open(path, "r") as f:
            cfg = json.load(f)
    except (OSError, ValueError) as e:
        raise OSError(f"cannot read {path}: {e}")
    return CTCSpec.from_config(cfg, name=ssl_type)
