"""Float64 statement of the reference's bimodal fusion head (oracle/fusion_head.py MultiModalEmotionClassifier), one utterance at a
time -- the reference's evaluation runs batch_size = 1, so no pad frame enters the recurrence, the attention or a pooling softmax.

``q`` names the operand rounding of the products the device runs on matrix cores (both operands of every such product):
  None      none: plain float64
  "f16x"    fp16 hi + lo      "fp32x"  bf16 hi + lo      "bf16"  bf16
With a ``q`` the recurrent product W_hh h always takes fp16 hi + lo operands (ser_gru_v's only form), h re-split every step.

Per case a test compares against three CPU quantities (``case_errors``): the float64 result, ``e_ref`` = the error of the oracle's own
fp32 arithmetic against it, ``e_split`` = the error of this statement with the mode's ``q`` against it.  Error form as everywhere:
max|a - b| / max(1, max|b|)."""
import numpy as np
import torch


def rel_err(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


def round_planes(x, q):
    """the operand planes of format ``q`` as float64: hi = cast, lo = cast of the remainder"""
    if q is None:
        return np.asarray(x, dtype=np.float64)
    t = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(torch.float32)          # operands are split from fp32 values
    if q == "bf16":
        return t.bfloat16().double().numpy()
    dt = torch.bfloat16 if q == "fp32x" else torch.float16
    hi = t.to(dt)
    lo = (t - hi.float()).to(dt)
    return (hi.double() + lo.double()).numpy()


class Rounded(np.ndarray):
    """a weight already in its operand format (``prepare`` rounds every matrix once per state dict, not once per product)"""


def mm(a, w, q):
    """a @ w.T with both operands in format ``q``"""
    return round_planes(a, q) @ (np.asarray(w) if isinstance(w, Rounded) else round_planes(w, q)).T


def _f64(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items() if k != "_prepared"}


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_direction(gx, w_hh, b_hh, reverse, rq):
    """gx [T, 3H] = x W_ih^T + b_ih of one direction; returns h [T, H].  ``rq``: operand format of W_hh h (None or "f16x")."""
    T, H = gx.shape[0], w_hh.shape[1]
    w = np.asarray(w_hh) if isinstance(w_hh, Rounded) else round_planes(w_hh, rq)
    h = np.zeros(H)
    out = np.zeros((T, H))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gh = w @ round_planes(h, rq)
        r = sigmoid(gx[t, :H] + gh[:H] + b_hh[:H])
        z = sigmoid(gx[t, H:2 * H] + gh[H:2 * H] + b_hh[H:2 * H])
        n = np.tanh(gx[t, 2 * H:] + r * (gh[2 * H:] + b_hh[2 * H:]))
        h = (1.0 - z) * n + z * h
        out[t] = h
    return out


def bigru_from_gx(gx, whh, bhh, rq=None):
    """gx [T, 6H] (forward gates | backward gates), whh [6H, H] = [weight_hh_l0 ; weight_hh_l0_reverse], bhh [6H] -> [T, 2H]"""
    gx, whh, bhh = (np.asarray(v, dtype=np.float64) for v in (gx, whh, bhh))
    H = whh.shape[1]
    return np.concatenate([gru_direction(gx[:, :3 * H], whh[:3 * H], bhh[:3 * H], False, rq),
                           gru_direction(gx[:, 3 * H:], whh[3 * H:], bhh[3 * H:], True, rq)], axis=1)


def bigru(x, sd, name, q):
    rq = None if q is None else "f16x"
    H = sd[f"{name}.weight_hh_l0"].shape[1]
    out = []
    for sfx, reverse in (("", False), ("_reverse", True)):
        gx = mm(x, sd[f"{name}.weight_ih_l0{sfx}"], q) + sd[f"{name}.bias_ih_l0{sfx}"]
        out.append(gru_direction(gx, sd[f"{name}.weight_hh_l0{sfx}"], sd[f"{name}.bias_hh_l0{sfx}"], reverse, rq))
    return np.concatenate(out, axis=1)


def xattn(qr, kr, vr, scale):
    """single-head attention between the projections: softmax_j(scale q . k_j) v_j, float64"""
    qr, kr, vr = (np.asarray(v, dtype=np.float64) for v in (qr, kr, vr))
    s = scale * (qr @ kr.T)
    s = s - s.max(axis=1, keepdims=True)
    p = np.exp(s)
    return (p / p.sum(axis=1, keepdims=True)) @ vr


def mha(xq, xkv, sd, name, q):
    E = xq.shape[1]
    w, b = sd[f"{name}.in_proj_weight"], sd[f"{name}.in_proj_bias"]
    qkv_q, qkv_kv = mm(xq, w, q), mm(xkv, w, q)                 # rows of in_proj_weight: q | k | v
    qr = qkv_q[:, :E] + b[:E]
    kr = qkv_kv[:, E:2 * E] + b[E:2 * E]
    vr = qkv_kv[:, 2 * E:] + b[2 * E:]
    ctx = xattn(qr, kr, vr, float(E) ** -0.5)
    return mm(ctx, sd[f"{name}.out_proj.weight"], q) + sd[f"{name}.out_proj.bias"]


def attn_pool(x, w, bias):
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64).reshape(-1)
    s = x @ w + float(bias)
    p = np.exp(s - s.max())
    return (p / p.sum()) @ x


def classifier(p, gamma, beta, w1, b1, w2, b2, eps=1e-5):
    p, gamma, beta, w1, b1, w2, b2 = (np.asarray(v, dtype=np.float64) for v in (p, gamma, beta, w1, b1, w2, b2))
    h = np.maximum(layer_norm(p, gamma, beta, eps) @ w1.T + b1, 0.0)
    return h @ w2.T + b2


MATRIX_CORE_WEIGHTS = ("projection.weight", "weight_ih_l0", "weight_ih_l0_reverse", "in_proj_weight", "out_proj.weight")


def prepare(sd, q):
    """the state dict in float64, the weights of the matrix-core products rounded to ``q`` once (W_hh to fp16 hi + lo whenever q is set)"""
    if isinstance(sd, dict) and sd.get("_prepared") == (q,):
        return sd
    out = _f64(sd)
    if q is not None:
        for k in list(out):
            if k.endswith(MATRIX_CORE_WEIGHTS):
                out[k] = round_planes(out[k], q).view(Rounded)
            elif "weight_hh_l0" in k:
                out[k] = round_planes(out[k], "f16x").view(Rounded)
    out["_prepared"] = (q,)
    return out


def head_logits(sd, x1, x2, q=None):
    """logits [n_out] of one utterance: x1 [T1, D1] speech rows, x2 [T2, D2] text rows"""
    sd = prepare(sd, q)
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    s = layer_norm(mm(x1, sd["speech_projection.weight"], q) + sd["speech_projection.bias"], sd["speech_norm.weight"], sd["speech_norm.bias"])
    t = layer_norm(mm(x2, sd["text_projection.weight"], q) + sd["text_projection.bias"], sd["text_norm.weight"], sd["text_norm.bias"])
    sh, th = bigru(s, sd, "speech_gru", q), bigru(t, sd, "text_gru", q)
    sa, ta = mha(sh, th, sd, "speech_attention", q), mha(th, sh, sd, "text_attention", q)
    ps = attn_pool(sh + sa, sd["speech_attn.weight"], sd["speech_attn.bias"][0])
    pt = attn_pool(th + ta, sd["text_attn.weight"], sd["text_attn.bias"][0])
    return classifier(np.concatenate([ps, pt])[None], sd["layer_norm.weight"], sd["layer_norm.bias"], sd["classifier.0.weight"],
                      sd["classifier.0.bias"], sd["classifier.3.weight"], sd["classifier.3.bias"])[0]


def batch_logits(sd, xs1, xs2, q=None):
    sd = prepare(sd, q)
    return np.stack([head_logits(sd, a, b, q) for a, b in zip(xs1, xs2)])


def oracle_model(sd, dtype=torch.float32):
    from oracle.fusion_head import MultiModalEmotionClassifier
    h = sd["speech_projection.weight"].shape[0]
    m = MultiModalEmotionClassifier(features1_dim=sd["speech_projection.weight"].shape[1], features2_dim=sd["text_projection.weight"].shape[1],
                                    fusion_hidden_dim=h, num_emotions=sd["classifier.3.weight"].shape[0])
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return m.to(dtype).eval()


def oracle_logits(sd, xs1, xs2, dtype=torch.float32):
    """oracle/fusion_head.py's module, each utterance as a batch of one"""
    m = oracle_model(sd, dtype)
    with torch.no_grad():
        return np.stack([m(torch.as_tensor(np.asarray(a)).to(dtype)[None], torch.as_tensor(np.asarray(b)).to(dtype)[None])[0].double().numpy()
                         for a, b in zip(xs1, xs2)])


def head_shapes(d1, d2, h=512, n_out=8):
    s = {"speech_projection.weight": (h, d1), "speech_projection.bias": (h,), "text_projection.weight": (h, d2), "text_projection.bias": (h,),
         "speech_norm.weight": (h,), "speech_norm.bias": (h,), "text_norm.weight": (h,), "text_norm.bias": (h,),
         "speech_attn.weight": (1, 2 * h), "speech_attn.bias": (1,), "text_attn.weight": (1, 2 * h), "text_attn.bias": (1,),
         "classifier.0.weight": (h, 4 * h), "classifier.0.bias": (h,), "classifier.3.weight": (n_out, h), "classifier.3.bias": (n_out,),
         "layer_norm.weight": (4 * h,), "layer_norm.bias": (4 * h,)}
    for g in ("speech_gru", "text_gru"):
        for sfx in ("", "_reverse"):
            s[f"{g}.weight_ih_l0{sfx}"] = (3 * h, h)
            s[f"{g}.weight_hh_l0{sfx}"] = (3 * h, h)
            s[f"{g}.bias_ih_l0{sfx}"] = (3 * h,)
            s[f"{g}.bias_hh_l0{sfx}"] = (3 * h,)
    for a in ("speech_attention", "text_attention"):
        s[f"{a}.in_proj_weight"] = (6 * h, 2 * h)
        s[f"{a}.in_proj_bias"] = (6 * h,)
        s[f"{a}.out_proj.weight"] = (2 * h, 2 * h)
        s[f"{a}.out_proj.bias"] = (2 * h,)
    return s


def seeded_case(d1, d2, lengths, seed, t2=80, h=512):
    """(state dict of torch fp32 tensors, speech rows per utterance, text rows per utterance), numpy PCG64"""
    from oracle.fusion_head import seeded_head_weights
    sd = seeded_head_weights(head_shapes(d1, d2, h), seed)
    g = np.random.default_rng(seed + 1000)
    xs1 = [g.standard_normal((t, d1), dtype=np.float32) for t in lengths]
    xs2 = [g.standard_normal((t2, d2), dtype=np.float32) for _ in lengths]
    return sd, xs1, xs2


_CACHE = {}


def case_errors(d1, d2, lengths, seed, q, t2=80):
    """(sd, xs1, xs2, float64 logits [B, 8], e_ref, e_split) -- computed once per case and shared"""
    key = (d1, d2, tuple(lengths), seed, t2)
    if key not in _CACHE:
        sd, xs1, xs2 = seeded_case(d1, d2, lengths, seed, t2)
        ref = batch_logits(sd, xs1, xs2)
        _CACHE[key] = dict(sd=sd, xs1=xs1, xs2=xs2, ref=ref, e_ref=rel_err(oracle_logits(sd, xs1, xs2), ref), split={})
    c = _CACHE[key]
    if q not in c["split"]:
        c["split"][q] = rel_err(batch_logits(c["sd"], c["xs1"], c["xs2"], q), c["ref"])
    return c["sd"], c["xs1"], c["xs2"], c["ref"], c["e_ref"], c["split"][q]
