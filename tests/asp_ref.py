"""Float64 statement of the organiser baseline's utterance-level tail, ragged and per utterance: attentive statistics pooling
(reference: benchmark/net/pooling.py AttentiveStatisticsPooling.forward) and the one-hidden-layer head (benchmark/net/ser.py
EmotionRegression in eval mode).  Written from the formulas; numpy only.

    h = tanh(x W^T + b);  s_t = h_t . a;  w = softmax_t(s)
    mu = sum_t w_t x_t;   rh = sqrt(max(sum_t w_t x_t^2 - mu^2, 1e-5));   pooled = [mu | rh]
    logits = W2 relu(LayerNorm_H(W1 pooled + b1; eps 1e-5) * gamma + beta) + b2
"""
import numpy as np

CLAMP = float(np.float32(1e-5))       # the reference clamps an fp32 tensor: the bound is the fp32 value of 1e-5


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def asp_scores(hlin, a):
    return np.tanh(_f64(hlin)) @ _f64(a).reshape(-1)


def asp_pool_from_scores(x, scores, frame_offs):
    """[B, 2 D]: the pooled rows of a packed ragged batch given the per-row scores."""
    x, scores = _f64(x), _f64(scores)
    out = np.empty((len(frame_offs) - 1, 2 * x.shape[1]))
    for b in range(len(frame_offs) - 1):
        xs, s = x[frame_offs[b]: frame_offs[b + 1]], scores[frame_offs[b]: frame_offs[b + 1]]
        w = np.exp(s - s.max())
        w = w / w.sum()
        mu = (w[:, None] * xs).sum(axis=0)
        var = (w[:, None] * xs * xs).sum(axis=0) - mu * mu
        out[b] = np.concatenate([mu, np.sqrt(np.maximum(var, CLAMP))])
    return out


def asp_pool(x, frame_offs, pool_sd, hlin=None):
    """Pooling with the weights of ``final_pool.pt``; ``hlin`` (x W^T + b, e.g. rounded to fp32 for a kernel test) may be given."""
    if hlin is None:
        hlin = _f64(x) @ _f64(pool_sd["sap_linear.weight"]).T + _f64(pool_sd["sap_linear.bias"])
    return asp_pool_from_scores(x, asp_scores(hlin, pool_sd["attention"]), frame_offs)


def mlp_head(p, ser_sd, eps=1e-5):
    """[B, n_out]: Linear -> LayerNorm (biased variance, eps inside the root) -> ReLU -> Linear."""
    h = _f64(p) @ _f64(ser_sd["fc.0.0.weight"]).T + _f64(ser_sd["fc.0.0.bias"])
    mean = h.mean(axis=1, keepdims=True)
    var = ((h - mean) ** 2).mean(axis=1, keepdims=True)
    y = (h - mean) / np.sqrt(var + eps) * _f64(ser_sd["fc.0.1.weight"]) + _f64(ser_sd["fc.0.1.bias"])
    return np.maximum(y, 0.0) @ _f64(ser_sd["out.0.weight"]).T + _f64(ser_sd["out.0.bias"])


def logits(x, frame_offs, pool_sd, ser_sd):
    return mlp_head(asp_pool(x, frame_offs, pool_sd), ser_sd)


def rel_err(got, ref):
    """max|got - ref| / max(1, max|ref|): the measure of tests/test_oracle_golden.py."""
    got, ref = _f64(got), _f64(ref)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))
