"""GPU: the speaker half of the 512-wide third stream -- ser_codec_unit_v, ser_codec_conv_v, ser_snake_v through the C ABI and
engine.SpeakerProsodyEncoder, the extraction driver and the scoring command -- against the float64 statement tests/codec_ref.py and the
reference's own run (tests/golden/tiny_codec_ngf8.npz).  Each test prints its numbers (lines starting CODEC).

Bounds.  Kernels and narrow levels: 4 x the fp32 torch twin's own distance from the statement on the same input -- both are fp32
evaluations of the same sums in a different order, so the same order of error is expected; the error form is max|a - b| / max(1, max|b|).
``encoded`` and the timbre rows: tests/test_gpu_e2e.py's gates (1e-3; bf16 3e-2).  hi + lo fp16 planes: 2^-21 max(1, max|.|).

Measured on an MI355X (profiles/codec.txt), error / twin error: ser_codec_unit_v 2.32 at worst (C = 8, d = 1, 15 rows: 2.3e-7 / 9.9e-8),
0.68-1.69 elsewhere; ser_codec_conv_v 0.73-1.68; ser_snake_v 0.94-1.00; the fixture's narrow levels 0.73-1.40.  encoded / timbre rows:
f16x 1.4e-6 / 1.2e-6, fp32x 1.1e-5 / 9.3e-6, bf16 5.9e-3 / 5.3e-3."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import codec_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEADS = 2
FACTOR = 4.0
TOL = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}          # tests/test_gpu_e2e.py TOL
ROWS = (3, 15, 75, 700)                                    # 3 and 15: shorter than any halo; 700: more than two time tiles


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _kmajor(w):
    """[N, C, k] -> [k * C, N]: the narrow kernels' weight layout"""
    return np.ascontiguousarray(np.transpose(w, (2, 1, 0)).reshape(-1, w.shape[0]), dtype=np.float32)


def _taps():
    from interspeech_ser_amd import prosody as P
    return _f32(P.kaiser_sinc_taps())


def _draw_conv(rng, n, c, k):
    """weights in the recipe of prosody.synthetic_codec_state_dict, as fp32 values: (w [N, C, k], bias)"""
    v = rng.standard_normal((n, c, k))
    return _f32(v * np.sqrt(0.5 / (c * k))), _f32(rng.uniform(-0.1, 0.1, n))


def _draw_act(rng, c):
    """(alpha, beta) fp32; the kernels get e^alpha and 1 / (e^beta + 1e-9) folded in float64 and rounded once, as prosody.prepare_codec"""
    return _f32(rng.uniform(-0.5, 0.5, c)), _f32(rng.uniform(-0.5, 0.5, c))


def _fold(act):
    a, b = act[0].astype(np.float64), act[1].astype(np.float64)
    return _f32(np.exp(a)), _f32(1.0 / (np.exp(b) + 1e-9))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


@pytest.fixture(scope="module")
def fx(built_library, golden_dir):
    """the fixture, the float64 statement and the fp32 twin of every wave (computed once)"""
    gold = R.load_golden(golden_dir)
    gold["stated"] = [R.forward(gold["enc"], gold["dec"], w, HEADS) for w in gold["waves"]]
    gold["twin"] = [R.torch_twin(gold["enc"], w) for w in gold["waves"]]
    dec = dict(gold["prosody"]["sd"])
    dec.update(gold["dec"])
    gold["dec_full"] = dec
    return gold


def _encoder(fx, mode, cache={}):
    from interspeech_ser_amd.engine import SpeakerProsodyEncoder
    if mode not in cache:
        cache[mode] = SpeakerProsodyEncoder(fx["dec_full"], fx["enc"], DEV, mode, heads=HEADS)
    return cache[mode]


# ----------------------------------------------------------------------------------------------------------------------- the unit
def _run_unit(xs, C, d, p, guard=5):
    """xs: list of [T, C] fp32 -> list of outputs; the batch sits ``guard`` rows into buffers with ``guard`` more rows behind it"""
    from interspeech_ser_amd import _lib
    offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]) + guard
    total = int(offs[-1]) + guard
    x = np.full((total, C), 7.0, dtype=np.float32)
    for b, v in enumerate(xs):
        x[offs[b]: offs[b + 1]] = v
    xd, yd = _dev(x), torch.full((total, C), -123.0, dtype=torch.float32, device=DEV)
    keep = [_dev(v) for v in (p["taps"], *_fold(p["act1"]), _kmajor(p["w7"]), p["b7"], *_fold(p["act2"]), _kmajor(p["w1"]), p["b1"])]
    od = _dev(offs, np.int32)
    a = _lib.CodecUnitArgs()
    a.x, a.y, a.row_offs = xd.data_ptr(), yd.data_ptr(), od.data_ptr()
    a.taps, a.ea1, a.ib1, a.w7, a.b7, a.ea2, a.ib2, a.w1, a.b1 = (t.data_ptr() for t in keep)
    a.B, a.C, a.k, a.dilation, a.max_rows, a.rows = len(xs), C, 7, d, max(len(v) for v in xs), total
    _lib.check(_lib.lib.ser_codec_unit_v(ctypes.byref(a), _stream()), "ser_codec_unit_v")
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[:guard] == -123.0).all() and (y[offs[-1]:] == -123.0).all()          # rows outside the batch are untouched
    return [y[offs[b]: offs[b + 1]] for b in range(len(xs))]


@pytest.mark.parametrize("C,d", [(8, 1), (8, 9), (32, 1), (32, 9)])
def test_unit_through_the_c_abi(built_library, C, d):
    from interspeech_ser_amd import _lib
    assert max(ROWS) > 2 * _lib.CODEC_TILE                                         # the longest utterance crosses at least two tiles
    rng = np.random.default_rng(100 * C + d)
    f = _taps()
    (w7, b7), (w1, b1) = _draw_conv(rng, C, C, 7), _draw_conv(rng, C, C, 1)
    p = dict(taps=f, act1=_draw_act(rng, C), act2=_draw_act(rng, C), w7=w7, b7=b7, w1=w1, b1=b1)
    xs = [_f32(rng.standard_normal((T, C))) for T in ROWS]
    got = _run_unit(xs, C, d, p)
    f64 = f.astype(np.float64)
    worst = 0.0
    for b, x in enumerate(xs):
        x64 = x.astype(np.float64)
        h = R.conv1d(R.activation1d(x64, *p["act1"], f64, f64), w7.astype(np.float64), b7.astype(np.float64), pad=3 * d, dilation=d)
        ref = x64 + R.conv1d(R.activation1d(h, *p["act2"], f64, f64), w1.astype(np.float64), b1.astype(np.float64))
        twin = R.twin_unit(_t(x.T)[None], _t(w7), _t(b7), _t(w1), _t(b1), d, (_t(p["act1"][0]), _t(p["act1"][1]), _t(f), _t(f)),
                           (_t(p["act2"][0]), _t(p["act2"][1]), _t(f), _t(f)))[0].T.numpy()
        e_twin, err = R.rel_err(twin, ref), R.rel_err(got[b], ref)
        print(f"CODEC unit C={C} d={d} rows={len(x)}: {err:.3e} (twin {e_twin:.3e}, ratio {err / e_twin:.2f})")
        worst = max(worst, err / e_twin)
        assert err <= FACTOR * e_twin
        alone = _run_unit([x], C, d, p, guard=0)[0]
        assert np.array_equal(_bits(alone), _bits(got[b]))                         # a batched run is bit-equal to a batch of one
    print(f"CODEC unit C={C} d={d}: worst ratio {worst:.2f}")


# ----------------------------------------------------------------------------------------------------------------------- the narrow convolution
def _run_conv(xs, out_rows, C_in, C_out, k, s, pad, w, b, act=None):
    from interspeech_ser_amd import _lib
    in_offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    out_offs = np.concatenate([[0], np.cumsum(out_rows)])
    xd = _dev(np.concatenate([np.asarray(x, dtype=np.float32).reshape(len(x), C_in) for x in xs]))
    total = int(out_offs[-1])
    yd = torch.full((total + 4, C_out), -123.0, dtype=torch.float32, device=DEV)
    keep = [_dev(_kmajor(w)), _dev(b), _dev(in_offs, np.int64), _dev(out_offs, np.int32)]
    a = _lib.CodecConvArgs()
    a.x, a.w, a.bias, a.in_offs, a.out_offs = xd.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr()
    if act is not None:
        keep += [_dev(_taps()), *(_dev(v) for v in _fold(act))]
        a.taps, a.ea, a.ib = keep[4].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr()
    a.y, a.ldy = yd.data_ptr(), C_out
    a.B, a.C_in, a.C_out, a.k, a.stride, a.pad, a.max_out_rows, a.rows = len(xs), C_in, C_out, k, s, pad, max(out_rows), total
    _lib.check(_lib.lib.ser_codec_conv_v(ctypes.byref(a), _stream()), "ser_codec_conv_v")
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[total:] == -123.0).all()
    return [y[out_offs[j]: out_offs[j + 1]] for j in range(len(xs))]


def test_conv_in_on_packed_unpadded_waves(fx):
    rng = np.random.default_rng(7)
    waves = fx["waves"][:3]                                                        # 400, 799 and 12 800 samples: the last gains a whole 200
    w, b = _draw_conv(rng, 32, 1, 7)
    P = [R.padded_len(len(x)) for x in waves]
    assert P == [600, 800, 13000]
    got = _run_conv(waves, P, 1, 32, 7, 1, 3, w, b)
    for j, x in enumerate(waves):
        xp = np.concatenate([x.astype(np.float64), np.zeros(P[j] - len(x))])[:, None]
        ref = R.conv1d(xp, w.astype(np.float64), b.astype(np.float64), pad=3)
        twin = torch.nn.functional.conv1d(_t(xp.T)[None], _t(w), _t(b), padding=3)[0].T.numpy()
        e_twin, err = R.rel_err(twin, ref), R.rel_err(got[j], ref)
        print(f"CODEC conv_in {len(x)} samples -> {P[j]} rows: {err:.3e} (twin {e_twin:.3e}, ratio {err / e_twin:.2f})")
        assert got[j].shape == (P[j], 32) and err <= FACTOR * e_twin
        tail = got[j][len(x) + 3:]                                                 # the implied zero tail: the bias alone
        assert np.array_equal(tail, np.broadcast_to(b, tail.shape)) and len(tail) == max(0, P[j] - len(x) - 3)
        assert np.array_equal(_bits(_run_conv([x], [P[j]], 1, 32, 7, 1, 3, w, b)[0]), _bits(got[j]))


@pytest.mark.parametrize("C,k,s,pad", [(8, 4, 2, 1), (16, 8, 4, 2), (32, 10, 5, 3)])
def test_activation_and_down_convolution(built_library, C, k, s, pad):
    rng = np.random.default_rng(10 * C + s)
    w, b = _draw_conv(rng, 2 * C, C, k)
    act = _draw_act(rng, C)
    xs = [_f32(rng.standard_normal((T * s, C))) for T in ROWS]                      # output rows 3, 15, 75, 700
    got = _run_conv(xs, list(ROWS), C, 2 * C, k, s, pad, w, b, act)
    f = _taps()
    f64 = f.astype(np.float64)
    for j, x in enumerate(xs):
        ref = R.conv1d(R.activation1d(x.astype(np.float64), *act, f64, f64), w.astype(np.float64), b.astype(np.float64), stride=s, pad=pad)
        twin = torch.nn.functional.conv1d(R.twin_activation1d(_t(x.T)[None], _t(act[0]), _t(act[1]), _t(f), _t(f)), _t(w), _t(b),
                                          stride=s, padding=pad)[0].T.numpy()
        e_twin, err = R.rel_err(twin, ref), R.rel_err(got[j], ref)
        print(f"CODEC act + down C={C} k={k} s={s} rows {len(x)} -> {len(ref)}: {err:.3e} (twin {e_twin:.3e}, ratio {err / e_twin:.2f})")
        assert ref.shape == (ROWS[j], 2 * C) and err <= FACTOR * e_twin
        assert np.array_equal(_bits(_run_conv([x], [ROWS[j]], C, 2 * C, k, s, pad, w, b, act)[0]), _bits(got[j]))


# ----------------------------------------------------------------------------------------------------------------------- the wide activation
SNAKE_ROWS, HALO = (3, 15, 130), 4


def _run_snake(xs, C, act, mode, rowmap=True):
    """-> (fp32 values per utterance, operand planes summed [all rows, C], plane tensor, halo'd row of every row, guard bits)"""
    from interspeech_ser_amd import _lib
    planes, dt = (2, torch.float16) if mode == _lib.MODE_FP16X else ((2, torch.bfloat16) if mode == _lib.MODE_FP32X else (1, torch.bfloat16))
    offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    total = int(offs[-1])
    rm = np.concatenate([np.arange(offs[b], offs[b + 1]) + HALO * (b + 1) for b in range(len(xs))]).astype(np.int32)
    out_rows = total + HALO * (len(xs) + 1)
    xd = _dev(np.concatenate(xs))
    actd = torch.zeros((planes, out_rows, C), dtype=torch.int16, device=DEV)
    f32 = torch.full((total, C), -123.0, dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    keep = [_dev(_taps()), *(_dev(v) for v in _fold(act)), _dev(offs, np.int32), _dev(rm, np.int32)]
    a = _lib.SnakeArgs()
    a.x, a.ldx, a.row_offs, a.taps, a.ea, a.ib = xd.data_ptr(), C, keep[3].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride = actd.data_ptr(), C, out_rows * C
    a.out_rowmap = keep[4].data_ptr() if rowmap else None
    a.out_f32, a.ldo_f32, a.range_flag = f32.data_ptr(), C, flag.data_ptr()
    a.B, a.C, a.max_rows, a.rows, a.mode = len(xs), C, max(len(x) for x in xs), total, mode
    _lib.check(_lib.lib.ser_snake_v(ctypes.byref(a), _stream()), "ser_snake_v")
    torch.cuda.synchronize()
    return f32.cpu().numpy(), actd.view(dt).float().cpu().numpy(), rm, int(flag.item())


@pytest.mark.parametrize("C", [64, 128])
def test_snake_values_planes_rowmap_and_range_guard(built_library, C):
    from interspeech_ser_amd import _lib
    rng = np.random.default_rng(C)
    act = _draw_act(rng, C)
    xs = [_f32(2.0 * rng.standard_normal((T, C))) for T in SNAKE_ROWS]
    f = _taps()
    f64 = f.astype(np.float64)
    ref = np.concatenate([R.activation1d(x.astype(np.float64), *act, f64, f64) for x in xs])
    twin = np.concatenate([R.twin_activation1d(_t(x.T)[None], _t(act[0]), _t(act[1]), _t(f), _t(f))[0].T.numpy() for x in xs])
    val, planes, rm, bits = _run_snake(xs, C, act, _lib.MODE_FP16X)
    e_twin, err = R.rel_err(twin, ref), R.rel_err(val, ref)
    print(f"CODEC snake C={C}: {err:.3e} (twin {e_twin:.3e}, ratio {err / e_twin:.2f})")
    assert bits == 0 and err <= FACTOR * e_twin
    both = planes.astype(np.float64).sum(axis=0)
    e_planes = float(np.abs(both[rm] - val.astype(np.float64)).max() / max(1.0, float(np.abs(val).max())))
    print(f"CODEC snake C={C}: hi + lo planes against the fp32 value {e_planes:.3e} (bound 2^-21 = {2.0 ** -21:.3e})")
    assert e_planes <= 2.0 ** -21
    halo = np.setdiff1d(np.arange(planes.shape[1]), rm)
    assert len(halo) == HALO * (len(xs) + 1) and not planes[:, halo].any()         # the halo rows stay zero
    val_b, planes_b, _, bits = _run_snake(xs, C, act, _lib.MODE_BF16)
    assert bits == 0 and np.array_equal(_bits(val_b), _bits(val))
    assert np.array_equal(planes_b[0][rm], torch.from_numpy(val).to(torch.bfloat16).float().numpy()) and not planes_b[:, halo].any()
    for j, x in enumerate(xs):                                                    # a batched run is bit-equal to a batch of one
        alone = _run_snake([x], C, act, _lib.MODE_FP16X)[0]
        lo = sum(SNAKE_ROWS[:j])
        assert np.array_equal(_bits(alone), _bits(val[lo: lo + len(x)]))
    # the fp16 range guard sees every value rounded to an fp16 plane, and only those
    big = [x.copy() for x in xs]
    big[2][:, 5] = 7.0e4                                                           # a constant channel: the activation passes its level
    assert _run_snake(big, C, act, _lib.MODE_FP16X)[3] == 3 and _run_snake(big, C, act, _lib.MODE_BF16)[3] == 0
    big[2][:, 5] = xs[2][:, 5]
    big[1][7, 9] = np.nan
    assert _run_snake(big, C, act, _lib.MODE_FP16X)[3] == 3 and _run_snake(big, C, act, _lib.MODE_BF16)[3] == 0


# -------------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_the_fixture(fx):
    from interspeech_ser_amd.engine import ProsodyEncoder
    g, offs, waves = fx["g"], fx["offs"], fx["waves"]
    narrow = ("conv_in", "u1_0", "u1_1", "u1_2", "level_1", "u2_0", "u2_1", "u2_2", "level_2", "u3_0", "u3_1", "u3_2", "level_3")
    levels = {}
    for mode in ("f16x", "fp32x", "bf16"):
        enc = _encoder(fx, mode)
        out = enc.forward(waves)
        assert out.frame_offs == [int(v) for v in offs] and [out.frames(b) for b in range(5)] == [3, 4, 65, 81, 130]
        rows, encoded = out.rows.cpu().numpy(), out.encoded.cpu().numpy()
        assert out.take_range_bits() == 0 and rows.shape == (283, 256) and rows.dtype == np.float32 and encoded.shape == (283, 128)
        plain = ProsodyEncoder(fx["prosody"]["sd"], DEV, mode, heads=HEADS).forward(waves)
        assert np.array_equal(_bits(rows[:, :128]), _bits(plain.rows.cpu().numpy())) and torch.equal(out.codes, plain.codes)
        e_enc = max(R.rel_err(encoded[offs[b]: offs[b + 1]], st["encoded"]) for b, st in enumerate(fx["stated"]))
        e_tim = max(R.rel_err(rows[offs[b]: offs[b + 1], 128:], st["timbre"]) for b, st in enumerate(fx["stated"]))
        e_fix = max(R.rel_err(encoded, g["encoded"]), R.rel_err(rows[:, 128:], g["timbre"]))
        print(f"CODEC {mode}: encoded {e_enc:.3e}, timbre rows {e_tim:.3e} against the statement (gate {TOL[mode]:.0e}); "
              f"against the reference's run {e_fix:.3e}")
        assert e_enc < TOL[mode] and e_tim < TOL[mode] and e_fix < TOL[mode]
        # every narrow level of the two short waves, one by one: the statement, the reference's run, and the other modes
        for b in (0, 1):
            lv = enc.forward([waves[b]], keep_levels=True).levels
            for name in narrow:
                got = lv[name].cpu().numpy()
                e_twin, err = R.rel_err(fx["twin"][b][name], fx["stated"][b][name]), R.rel_err(got, fx["stated"][b][name])
                print(f"CODEC {mode} wave {b} {name}: {err:.3e} (twin {e_twin:.3e}, ratio {err / e_twin:.2f})")
                assert err <= FACTOR * e_twin, (mode, b, name)
                if f"lv{b}.{name}" in g:
                    assert R.rel_err(got, g[f"lv{b}.{name}"]) <= FACTOR * e_twin + R.rel_err(g[f"lv{b}.{name}"], fx["stated"][b][name])
                assert np.array_equal(_bits(got), levels.setdefault((b, name), _bits(got))), (mode, b, name)   # mode-independent
        # a batched run is bit-equal to a batch of one, per wave
        for b in (0, 1, 3):
            alone = enc.forward([waves[b]])
            assert np.array_equal(_bits(alone.rows.cpu().numpy()), _bits(rows[offs[b]: offs[b + 1]])), (mode, b)
            assert np.array_equal(_bits(alone.encoded.cpu().numpy()), _bits(encoded[offs[b]: offs[b + 1]]))


def test_full_geometry_on_two_short_waves(built_library):
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.engine import SpeakerProsodyEncoder
    import prosody_ref as RP
    dec = P.synthetic_state_dict(seed=11)
    dec.update(P.synthetic_timbre_state_dict(seed=13))
    enc_sd = P.synthetic_codec_state_dict()
    rng = np.random.default_rng(12)
    waves = [(0.3 * np.sin(np.arange(n) * f) + 0.05 * rng.standard_normal(n)).astype(np.float32) for n, f in ((1000, 0.11), (3333, 0.07))]
    enc = SpeakerProsodyEncoder(dec, enc_sd, DEV, "f16x")
    sp = enc.spec
    assert sp == P.CodecSpec() and (sp.ngf, sp.strides, sp.out_channels, sp.hidden, sp.hop) == (32, (2, 4, 5, 5), 256, 512, 200)
    assert (sp.timbre.hidden, sp.timbre.num_layers, sp.timbre.ffn, sp.timbre.kernel, sp.timbre.heads) == (256, 4, 1024, 5, 4)
    out = enc.forward(waves)
    rows, encoded = out.rows.cpu().numpy(), out.encoded.cpu().numpy()
    assert out.frame_offs == [0, 6, 23] and out.take_range_bits() == 0 and rows.shape == (23, 512)
    for j, w in enumerate(waves):
        sl = slice(out.frame_offs[j], out.frame_offs[j + 1])
        st = R.forward(enc_sd, dec, w, 4)
        pro = RP.forward(dec, w, 4)
        e_enc, e_tim = R.rel_err(encoded[sl], st["encoded"]), R.rel_err(rows[sl, 256:], st["timbre"])
        sure = pro["gaps"] > 1e-3                                                  # (a frame under the gap may take a neighbouring code)
        result = np.concatenate([pro["rows"], st["timbre"]], axis=1)
        e_res = R.rel_err(rows[sl][sure], result[sure])
        print(f"CODEC full geometry wave {j}: encoded {e_enc:.3e}, timbre {e_tim:.3e}, result {e_res:.3e} (gate 1e-3); max|encoded| {np.abs(st['encoded']).max():.2f}")
        assert e_enc < 1e-3 and e_tim < 1e-3 and e_res < 1e-3


def test_replay_equals_a_fresh_eager_forward(fx):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import SpeakerProsodyEncoder
    waves = fx["waves"]
    eager = SpeakerProsodyEncoder(fx["dec_full"], fx["enc"], DEV, "f16x", heads=HEADS)
    eager.use_tape = False
    taped = _encoder(fx, "f16x")
    # slot 0: recorded once, on the largest batch, sizes patched for the others.  Slot 1 starts small: the arena grows under a recorded list
    # (which must be recorded again over the new buffers), then holds a subset and the full batch again
    runs = [(batch, 0) for batch in (waves, [waves[3], waves[0]], [waves[1]], waves)]
    runs += [(batch, 1) for batch in ([waves[1]], waves, [waves[3], waves[0]], waves)]
    for batch, slot in runs:
        a, b = eager.forward(batch, slot=slot), taped.forward(batch, slot=slot)
        lens = [len(w) for w in batch]
        assert taped.recorded_tape(lens, slot).n > 0
        with pytest.raises(_lib.SerHipError, match="no recorded command list"):
            eager.recorded_tape(lens, slot)
        _same_features(a, b)
    # only the INNER prosody encoder's arena grows between two forwards of the outer one: the outer list points into it as well
    small, larger = [waves[1]], waves
    want = eager.forward(small, slot=2)
    first = taped.forward(small, slot=2)
    _same_features(want, first)
    taped.prosody.forward(larger, slot=2)
    _same_features(eager.forward(small, slot=2), taped.forward(small, slot=2))


def _same_features(a, b):
    for name in ("rows", "encoded", "z", "gaps", "mel"):
        assert np.array_equal(_bits(getattr(a, name).cpu().numpy()), _bits(getattr(b, name).cpu().numpy())), name
    assert torch.equal(a.codes, b.codes) and a.frame_offs == b.frame_offs
    assert a.take_range_bits() == 0 and b.take_range_bits() == 0


def test_short_wave_fails_alone(fx):
    enc = _encoder(fx, "f16x")
    with pytest.raises(ValueError, match="400 samples"):
        enc.forward([fx["waves"][0], fx["prosody"]["short"]])
    assert enc.forward([fx["waves"][0]]).frame_offs == [0, 3]


# --------------------------------------------------------------------------------------------------------------------- drivers
def _write_wav(path, x):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.round(np.asarray(x, dtype=np.float64) * 32768.0).astype("<i2").tobytes())


def test_driver_writes_the_reference_files(fx, tmp_path, capsys):
    from interspeech_ser_amd import prosody as P
    enc = _encoder(fx, "f16x")
    wav_dir, out = tmp_path / "Audios", tmp_path / "ns3"
    wav_dir.mkdir()
    picks = {"a.wav": fx["waves"][1], "b.wav": fx["waves"][3], "short.wav": fx["prosody"]["short"], "c.wav": fx["waves"][0]}
    for name, w in picks.items():
        _write_wav(wav_dir / name, w)                                              # int16 PCM / 32768: the fixture's waves exactly
    assert P.run_speaker(["--wav_dir", str(wav_dir), "--save_path", str(out), "--num_workers", "2", "--batch_size", "3"], encoder=enc) == 0
    log = capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["a.pt", "b.pt", "c.pt"], log
    assert log.count("Failed to process") == 1 and f"Failed to process {wav_dir / 'short.wav'}" in log and "400 samples" in log, log
    for name, w in picks.items():
        if name == "short.wav":
            continue
        t = torch.load(out / name.replace(".wav", ".pt"), weights_only=True)
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(w) // 200 + 1, 256)
        assert torch.equal(t, enc.forward([w]).rows.cpu())


def test_scoring_from_wav_equals_the_route_through_the_drivers_files(built_library, tmp_path, capsys):
    """bin/predict_cat_from_wav.py --encoder3 ns3-prosody-speaker on synthetic weights writes, byte for byte, the results/test.csv that
    the driver's .pt files give through --encoder3 files in the same modes."""
    import pandas as pd
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.predictor import score_from_wav
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import synth_wave
    import fusion3_ref as R3
    geo, max_len = C.TINY_ROBERTA, 16
    wav_dir, lazy3 = tmp_path / "Audios", tmp_path / "ns3"
    wav_dir.mkdir()
    lengths = (4800, 6400, 399, 3000)
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(len(lengths))]
    for i, (name, n) in enumerate(zip(names, lengths)):
        _write_wav(wav_dir / name, 0.5 * synth_wave(40 + i, n))
    texts = ["hello there", "a longer sentence with more words", "too short to pad", "yes no"]
    pd.DataFrame({"FileName": names, "transcription": texts}).to_csv(tmp_path / "text.csv", index=False)
    pd.DataFrame({"FileName": names}).to_csv(tmp_path / "test.csv", index=False)

    def fake_tokenize(batch):
        ids = torch.full((len(batch), max_len), geo.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((len(batch), max_len), dtype=torch.int64)
        for i, t in enumerate(batch):
            toks = ([0] + [3 + (len(w) * 7 + j) % (geo.vocab_size - 4) for j, w in enumerate(t.split())])[: max_len - 1] + [2]
            ids[i, : len(toks)] = torch.tensor(toks)
            mask[i, : len(toks)] = 1
        return ids, mask

    sd = seeded_head_weights(R3.head_shapes(320, 128, 512, h=64), 31)
    cfgs = []
    for tag in ("files", "wav"):
        cfg = {"wav_dir": str(wav_dir), "txt_dir": str(tmp_path / "text.csv"), "lazy_dir3": str(lazy3), "feat1_dim": 320, "feat2_dim": 128,
               "feat3_dim": 512, "model_path": str(tmp_path / f"exp_{tag}")}
        os.makedirs(cfg["model_path"])
        torch.save(sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
        cfgs.append(cfg)
    C._REGISTRY["tiny-hubert-speaker"], C._REGISTRY["tiny-roberta-speaker"] = C.TINY_HUBERT, geo
    streams = ["tiny-hubert-speaker", "tiny-roberta-speaker"]
    common = dict(test_csv=str(tmp_path / "test.csv"), mode="f16x", text_mode="f16x", head_mode="f16x", batch_size=2, max_len=max_len,
                  synthetic_weights=True, tokenize=fake_tokenize)                   # batches [0, 1], [2, 3]: file 3 runs alone on both routes
    try:
        assert P.run_speaker(["--wav_dir", str(wav_dir), "--save_path", str(lazy3), "--synthetic_weights", "--mode", "f16x", "--batch_size", "2"]) == 0
        assert sorted(os.listdir(lazy3)) == [n.replace(".wav", ".pt") for n in names if n != names[2]]
        assert tuple(torch.load(lazy3 / "MSP-PODCAST_0001.pt", weights_only=True).shape) == (33, 512)
        capsys.readouterr()
        a = score_from_wav(cfgs[0], streams + ["files"], **common)
        log_a = capsys.readouterr().out
        b = score_from_wav(cfgs[1], streams + [P.NS3_PROSODY_SPEAKER], **common)
        log_b = capsys.readouterr().out
        with pytest.raises(ValueError, match="feat3_dim = 256 in the config, but ns3-prosody-speaker has hidden size 512"):
            score_from_wav(dict(cfgs[1], feat3_dim=256), streams + [P.NS3_PROSODY_SPEAKER], **common)
    finally:
        C._REGISTRY.pop("tiny-hubert-speaker")
        C._REGISTRY.pop("tiny-roberta-speaker")
    for res, log in ((a, log_a), (b, log_b)):
        assert res["n"] == 3 and res["failed"] == 1, log
        assert log.count("Failed to process") == 1 and "Failed to process MSP-PODCAST_0002.wav" in log, log
    assert "Stream 3: ns3-prosody-speaker (synthetic weights (seed 7); numerics mode f16x)" in log_b
    with open(a["csv"], "rb") as f:
        by_files = f.read()
    with open(b["csv"], "rb") as f:
        from_wav = f.read()
    assert from_wav == by_files
    assert [ln.split(",")[0] for ln in from_wav.decode().splitlines()[1:]] == [names[0], names[1], names[3]]
