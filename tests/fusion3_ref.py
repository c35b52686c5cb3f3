"""Float64 statement of the reference's trimodal fusion head (head.TrimodalEmotionClassifier: speech, text and a third stream under the
``prosody_*`` names), one utterance at a time -- the reference's scoring scripts run batch_size = 1.  Built from the functions of
tests/fusion_ref.py plus a multi-head ``mha``; ``q`` is the same operand-rounding hook (None, "f16x", "fp32x", "bf16").

Each attention module serves both pairs of its query side, as the reference shares them; ``heads`` = the modules' head counts, (1, 1, 2) in
the reference.  ``case_errors`` gives, per case, the float64 logits, ``e_ref`` (the fp32 torch class against them) and ``e_split`` (this
statement with the mode's ``q`` against them)."""
import numpy as np
import torch

import fusion_ref as R

NAMES = ("speech", "text", "prosody")
HEADS = (1, 1, 2)


def mha(xq, xkv, sd, name, q, heads=1):
    """nn.MultiheadAttention(E, heads) of module ``name``: head h is columns h dh .. (h+1) dh - 1 of the projections, scale dh^-0.5"""
    E = xq.shape[1]
    dh = E // heads
    w, b = sd[f"{name}.in_proj_weight"], sd[f"{name}.in_proj_bias"]
    qkv_q, qkv_kv = R.mm(xq, w, q), R.mm(xkv, w, q)               # rows of in_proj_weight: q | k | v
    qr = qkv_q[:, :E] + b[:E]
    kr = qkv_kv[:, E:2 * E] + b[E:2 * E]
    vr = qkv_kv[:, 2 * E:] + b[2 * E:]
    ctx = np.concatenate([R.xattn(qr[:, h * dh:(h + 1) * dh], kr[:, h * dh:(h + 1) * dh], vr[:, h * dh:(h + 1) * dh], float(dh) ** -0.5)
                          for h in range(heads)], axis=1)
    return R.mm(ctx, sd[f"{name}.out_proj.weight"], q) + sd[f"{name}.out_proj.bias"]


def head_logits(sd, x1, x2, x3, q=None, heads=HEADS):
    """logits [n_out] of one utterance: x1 [T1, D1] speech rows, x2 [T2, D2] text rows, x3 [T3, D3] (or [T3, D3, 1]) third-stream rows"""
    sd = R.prepare(sd, q)
    xs = [np.asarray(x, dtype=np.float64) for x in (x1, x2, x3)]
    if xs[2].ndim == 3:
        xs[2] = xs[2][..., 0]
    hid = []
    for name, x in zip(NAMES, xs):
        p = R.layer_norm(R.mm(x, sd[f"{name}_projection.weight"], q) + sd[f"{name}_projection.bias"], sd[f"{name}_norm.weight"], sd[f"{name}_norm.bias"])
        hid.append(R.bigru(p, sd, f"{name}_gru", q))
    pooled = []
    for i, name in enumerate(NAMES):
        final = hid[i]
        for j in range(3):
            if j != i:
                final = final + mha(hid[i], hid[j], sd, f"{name}_attention", q, heads[i])
        pooled.append(R.attn_pool(final, sd[f"{name}_attn.weight"], sd[f"{name}_attn.bias"][0]))
    return R.classifier(np.concatenate(pooled)[None], sd["layer_norm.weight"], sd["layer_norm.bias"], sd["classifier.0.weight"],
                        sd["classifier.0.bias"], sd["classifier.3.weight"], sd["classifier.3.bias"])[0]


def batch_logits(sd, xs1, xs2, xs3, q=None, heads=HEADS):
    sd = R.prepare(sd, q)
    return np.stack([head_logits(sd, a, b, c, q, heads) for a, b, c in zip(xs1, xs2, xs3)])


def head_shapes(d1, d2, d3, h=512, n_out=8):
    """state-dict keys -> shapes, in the order of the reference class"""
    s = {}
    for name, d in zip(NAMES, (d1, d2, d3)):
        s[f"{name}_projection.weight"], s[f"{name}_projection.bias"] = (h, d), (h,)
    for name in NAMES:
        s[f"{name}_norm.weight"], s[f"{name}_norm.bias"] = (h,), (h,)
    for name in NAMES:
        for sfx in ("", "_reverse"):
            s[f"{name}_gru.weight_ih_l0{sfx}"] = (3 * h, h)
            s[f"{name}_gru.weight_hh_l0{sfx}"] = (3 * h, h)
            s[f"{name}_gru.bias_ih_l0{sfx}"] = (3 * h,)
            s[f"{name}_gru.bias_hh_l0{sfx}"] = (3 * h,)
    for name in NAMES:
        s[f"{name}_attention.in_proj_weight"], s[f"{name}_attention.in_proj_bias"] = (6 * h, 2 * h), (6 * h,)
        s[f"{name}_attention.out_proj.weight"], s[f"{name}_attention.out_proj.bias"] = (2 * h, 2 * h), (2 * h,)
    for name in NAMES:
        s[f"{name}_attn.weight"], s[f"{name}_attn.bias"] = (1, 2 * h), (1,)
    s.update({"classifier.0.weight": (h, 6 * h), "classifier.0.bias": (h,), "classifier.3.weight": (n_out, h), "classifier.3.bias": (n_out,),
              "layer_norm.weight": (6 * h,), "layer_norm.bias": (6 * h,)})
    return s


def seeded_rows(dims, lengths, seed):
    """per modality, the rows of each utterance: ``lengths`` = (speech lengths, text lengths, third-stream lengths), numpy PCG64"""
    g = np.random.default_rng(seed)
    return [[g.standard_normal((t, d), dtype=np.float32) for t in ln] for d, ln in zip(dims, lengths)]


def seeded_case(dims, lengths, seed, h=512):
    """(state dict of torch fp32 tensors, speech rows, text rows, third-stream rows)"""
    from oracle.fusion_head import seeded_head_weights
    sd = seeded_head_weights(head_shapes(*dims, h=h), seed)
    return (sd, *seeded_rows(dims, lengths, seed + 1000))


def torch_model(sd, dtype=torch.float32):
    from interspeech_ser_amd.head import TrimodalEmotionClassifier
    m = TrimodalEmotionClassifier(*(sd[f"{n}_projection.weight"].shape[1] for n in NAMES), fusion_hidden_dim=sd["speech_projection.weight"].shape[0],
                                  num_emotions=sd["classifier.3.weight"].shape[0])
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return m.to(dtype).eval()


def torch_logits(sd, xs1, xs2, xs3, dtype=torch.float32):
    """head.TrimodalEmotionClassifier (pinned to the reference's class by tests/golden/trimodal_head_pins.npz), each utterance as a batch of one"""
    m = torch_model(sd, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)[None]
    with torch.no_grad():
        return np.stack([m(t(a), t(b), t(c))[0].double().numpy() for a, b, c in zip(xs1, xs2, xs3)])


_CACHE = {}


def case_errors(dims, lengths, seed, q, h=512):
    """(sd, xs1, xs2, xs3, float64 logits [B, 8], e_ref, e_split) -- computed once per case and shared"""
    key = (tuple(dims), tuple(tuple(ln) for ln in lengths), seed, h)
    if key not in _CACHE:
        sd, xs1, xs2, xs3 = seeded_case(dims, lengths, seed, h)
        ref = batch_logits(sd, xs1, xs2, xs3)
        _CACHE[key] = dict(sd=sd, xs=(xs1, xs2, xs3), ref=ref, e_ref=R.rel_err(torch_logits(sd, xs1, xs2, xs3), ref), split={})
    c = _CACHE[key]
    if q not in c["split"]:
        c["split"][q] = R.rel_err(batch_logits(c["sd"], *c["xs"], q), c["ref"])
    return (c["sd"], *c["xs"], c["ref"], c["e_ref"], c["split"][q])
