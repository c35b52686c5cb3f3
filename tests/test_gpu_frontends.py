"""-m gpu: the two kernels every utterance passes through first, ser_logmel_whisper (csrc/logmel.hip) and ser_wave_frames_v
(csrc/rowops.hip), through the C ABI against the float64 statements of tests/frontend_ref.py (pinned to the Hugging Face probes and the
oracles by tests/test_frontend_ref_host.py).  Every gate is the reference's own distance from the statement on the same wave (e_ref, times
the project's usual 2) plus what the number formats of the kernel's remaining fp32 / 16-bit stages allow; none is a fitted constant.
Each test prints its measured figures in lines that start with "FRONTENDS64" (profiles/frontends_float64.txt keeps one run of them)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import base_oracle as BO
import frontend_ref as R
from test_gpu_kernels import to_act                      # bf16 one plane / bf16 hi + lo, the suite's host restatement of the split
from test_gpu_range_guard import planes as f16_planes    # fp16 hi + lo, likewise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, FP32X, FP16X = 1, 2, 4
MODE_NAME = {BF16: "bf16", FP32X: "fp32x", FP16X: "fp16x"}

U32 = 2.0 ** -24                                         # unit roundoff of fp32 (24-bit significand)


def ulp32(v):
    """spacing of fp32 at magnitude v"""
    return float(np.spacing(np.float32(v)))


# What the fp32 stages that follow the fp64 DFT may add to a feature, from the formats alone:
#   re, im rounded to fp32 (u32 each, 2 u32 on a square), one rounding per square and one for their sum       power bin: 4 u32 relative
#   201 FMAs into one accumulator, one rounding each, all terms non-negative (no cancellation)                 mel power: + 201 u32 relative
#   log10 of a value that is off by r relatively moves by r / ln 10                                            205 u32 / ln 10 = 5.31e-6
#   log10f itself: 2 ulp (HIP math API), |v| <= 10 so ulp <= 2^-20                                              + 1.91e-6
#   the clamp max - 8 (|.| < 16: half an ulp of 2^-20) and v + 4 (|.| < 8: half an ulp of 2^-21)                + 4.8e-7 + 2.4e-7
#   / 4 is exact and scales all of it                                                                          1.98e-6
LOGMEL_FLOOR = ((4 + 201) * U32 / math.log(10.0) + 2 * ulp32(10.0) + 0.5 * ulp32(15.0) + 0.5 * ulp32(7.0)) / 4.0


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(line):
    print("FRONTENDS64 " + line)


# ------------------------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def mel_matrix(n_mels):
    """[201, n_mels] fp32: Whisper's filters for 80 and 128; 160 is a seeded non-negative matrix of their scale (no Whisper has that many:
    it is there for the second pass of the kernel's m += 128 loop)."""
    from interspeech_ser_amd.frontend import whisper_mel_filters
    if n_mels in (80, 128):
        return whisper_mel_filters(n_mels)
    return (0.03 * np.random.default_rng(n_mels).random((R.N_BINS, n_mels))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_waves(name):
    return tuple(R.logmel_case(name))


@functools.lru_cache(maxsize=None)
def power_of(name, i):
    return R.power64(case_waves(name)[i])


def fp32_log_mel(wave, mel):
    """oracle.whisper_log_mel's fp32 pipeline for an arbitrary filter matrix (the oracle builds its own from n_mels)."""
    x = np.zeros(R.N_SAMPLES, dtype=np.float32)
    w = np.asarray(wave, dtype=np.float32)[:R.N_SAMPLES]
    x[: len(w)] = w
    frames = F.pad(torch.from_numpy(x)[None, None], (200, 200), mode="reflect")[0, 0].unfold(0, 400, 160)
    spec = torch.fft.rfft(frames * torch.hann_window(400, periodic=True, dtype=torch.float32), n=400, dim=-1)
    power = (spec.real ** 2 + spec.imag ** 2)[:-1].transpose(0, 1)
    log_spec = torch.clamp(torch.from_numpy(mel).transpose(0, 1) @ power, min=1e-10).log10()
    return ((torch.maximum(log_spec, log_spec.max() - 8.0) + 4.0) / 4.0).numpy()


@functools.lru_cache(maxsize=None)
def logmel_reference(name, i, n_mels):
    """(float64 statement, e_ref = max |fp32 reference - statement|) of wave i of a case: no code under test is involved."""
    from oracle import ssl_oracle as O
    wave, mel = case_waves(name)[i], mel_matrix(n_mels)
    ref = R.log_mel64(wave, mel, power_of(name, i))
    ref.setflags(write=False)
    fp32 = O.whisper_log_mel(wave, n_mels) if n_mels in (80, 128) else fp32_log_mel(wave, mel)
    return ref, float(np.abs(fp32.astype(np.float64) - ref).max())


# --------------------------------------------------------------------------------------------------------------------------- ser_logmel_whisper
CANARY = 12345.0


def new_logmel_work(L, B):
    work = torch.zeros(L.lib.ser_workspace_bytes(L.WS_LOGMEL, B, 0, 0, 0, 1), dtype=torch.uint8, device=DEV)
    L.check(L.lib.ser_logmel_init(work.data_ptr(), B, stream()), "ser_logmel_init")
    return work


def run_logmel(L, waves, n_mels, work=None):
    """[B, n_mels, 3000] fp32 (CPU tensor) of one launch over the ragged batch.  The output sits between two rows of 64 canary floats and
    starts as NaN: the launch has to write all of it and nothing else."""
    B = len(waves)
    lens = [len(w) for w in waves]
    packed = torch.from_numpy(np.concatenate(list(waves) + [np.zeros(1, dtype=np.float32)])).to(DEV)     # + 1: never an empty allocation
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    mel = torch.from_numpy(mel_matrix(n_mels)).to(DEV)
    n = B * n_mels * R.N_FRAMES
    buf = torch.full((64 + n + 64,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:64] = CANARY
    buf[64 + n:] = CANARY
    if work is None:
        work = new_logmel_work(L, B)
    L.check(L.lib.ser_logmel_whisper(packed.data_ptr(), offs.data_ptr(), B, mel.data_ptr(), n_mels, buf.data_ptr() + 64 * 4,
                                     work.data_ptr(), stream()), "ser_logmel_whisper")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:64] == CANARY).all()) and bool((host[64 + n:] == CANARY).all()), "ser_logmel_whisper wrote outside its output"
    out = host[64: 64 + n].reshape(B, n_mels, R.N_FRAMES)
    assert not bool(torch.isnan(out).any()), "ser_logmel_whisper left part of its output unwritten"
    return out


@pytest.mark.parametrize("n_mels", [80, 128, 160])
@pytest.mark.parametrize("name", R.LOGMEL_CASES)
def test_logmel_equals_the_float64_statement(L, name, n_mels):
    """max |kernel - log_mel64| <= 2 e_ref + LOGMEL_FLOOR for every utterance of every case: e_ref is the fp32 reference's own distance
    from the statement on that wave, LOGMEL_FLOOR (derived above) what the kernel's fp32 stages after the fp64 DFT may add."""
    waves = case_waves(name)
    got = run_logmel(L, waves, n_mels).numpy().astype(np.float64)
    failures = []
    for i, w in enumerate(waves):
        ref, e_ref = logmel_reference(name, i, n_mels)
        err = np.abs(got[i] - ref)
        gate = 2.0 * e_ref + LOGMEL_FLOOR
        at = np.unravel_index(int(err.argmax()), err.shape)
        record(f"logmel {name}[{len(w)} samples] n_mels {n_mels}: kernel {float(err.max()):.3e} e_ref {e_ref:.3e} gate {gate:.3e} "
               f"(worst at mel {at[0]} frame {at[1]}, statement {float(ref[at]):+.6f})")
        if not float(err.max()) <= gate:
            failures.append((len(w), float(err.max()), gate))
        if name == "silence":
            assert bool((got[i] == -1.5).all()), "silence is the 1e-10 guard everywhere: (-10 + 4) / 4"
    assert not failures, failures


def test_logmel_batch_neighbours_do_not_move_the_clamp(L):
    """Each utterance's max - 8 floor comes from its own 94 block maxima: a batch is its utterances one by one, bit for bit (no atomics)."""
    waves = [case_waves("loud then quiet")[0], case_waves("silence")[0], case_waves("tone over floor")[0], np.full(1, 0.01, dtype=np.float32)]
    for n_mels in (80, 160):
        batch = run_logmel(L, waves, n_mels)
        for i, w in enumerate(waves):
            alone = run_logmel(L, [w], n_mels)
            assert torch.equal(batch[i].view(torch.int32), alone[0].view(torch.int32)), (n_mels, i)
        assert float(batch[3].max()) < float(batch[0].max()) - 1.0       # the 1-sample clip's own range lies far below its neighbours'


def test_logmel_work_buffer_reuse_across_batch_sizes(L):
    """ser_logmel_init once, then B = 4 (loud) and B = 2 (quiet, other waves) on the same buffer: the maxima slots are never reset, so
    the second call must overwrite every slot it reads.  It equals the same call on a fresh buffer."""
    rng = np.random.default_rng(12)
    loud = [np.clip(0.9 * rng.standard_normal(n), -1, 1).astype(np.float32) for n in (480000, 16000, 3000, 100000)]
    quiet = [(1e-4 * rng.standard_normal(n)).astype(np.float32) for n in (20000, 1)]
    work = new_logmel_work(L, 4)
    first = run_logmel(L, loud, 80, work)
    second = run_logmel(L, quiet, 80, work)
    fresh = run_logmel(L, quiet, 80)
    assert torch.equal(second.view(torch.int32), fresh.view(torch.int32))
    assert torch.equal(run_logmel(L, loud, 80, work).view(torch.int32), first.view(torch.int32))
    assert float(second.max()) < float(first.max()) - 1.0


@pytest.mark.parametrize("n_mels", [80, 160])
def test_logmel_writes_its_output_and_nothing_else(L, n_mels):
    """Canaries on both sides and a NaN prefill (run_logmel asserts both): the last frame block holds frames 2976 .. 3007, its guard is
    per quad, and n_mels = 80 / 160 leave 48 / 96 of the 128 mel lanes of a pass idle.  Every value lies in [max - 2, max] of its
    utterance: the 8-decade clamp after (v + 4) / 4.  Both ends are fp32 results: the floor is fl(fl(fl(max - 8) + 4) / 4), the top
    fl(fl(max + 4) / 4), so their distance is 2 up to half an ulp of max - 8 (|.| < 16: 2^-21) and half an ulp of each v + 4
    (|.| < 8: 2^-22 each), a quarter of it after the exact division: 2^-22."""
    slack = (0.5 * ulp32(15.0) + 2 * 0.5 * ulp32(7.0)) / 4.0
    waves = [case_waves("30 s truncated")[0], case_waves("noise")[0][:1234], case_waves("DC offset")[0]]
    out = run_logmel(L, waves, n_mels)
    for i in range(len(waves)):
        top = float(out[i].max())
        assert float(out[i].min()) >= top - 2.0 - slack and math.isfinite(top), (i, float(out[i].min()), top)


# ---------------------------------------------------------------------------------------------------------------------------- ser_wave_frames_v
K, STRIDE = 10, 5
PRE, POST = 3, 5                                          # canary rows before and after the frames, in every plane
FILL = 0x7B7B                                             # bf16 1.3e36 / fp16 61280: no kernel output looks like it


def unit_roundoff(mode):
    """(u, eta) of the operand format: a value v is held as v (1 + d) + e with |d| <= u, |e| <= eta.  u = half the format's epsilon for
    one plane, its square for hi + lo (lo holds the rounded remainder of hi); eta = half the spacing of the format's subnormals, which a
    plane cannot resolve (fp16: 2^-25; it only shows where v or its remainder falls below 2^-14)."""
    dt = torch.float16 if mode == FP16X else torch.bfloat16
    half_eps = torch.finfo(dt).eps / 2.0
    return (half_eps if mode == BF16 else half_eps * half_eps), torch.finfo(dt).smallest_normal * torch.finfo(dt).eps / 2.0


def host_planes(x32, mode):
    """fp32 CPU [rows, 64] -> the planes the suite's helpers split it into, as int16 words on the CPU"""
    p = f16_planes(x32, FP16X) if mode == FP16X else to_act(x32, mode)
    return p.cpu().view(torch.int16)


@functools.lru_cache(maxsize=None)
def wave_reference(name):
    """per clip: (fp32 samples, normalised float64 statement, e_ref = max |base_oracle.normalize_wave - statement|)"""
    out = []
    for w in R.wave_case(name):
        ref = R.wave_norm64(w)
        out.append((w, ref, float(np.abs(BO.normalize_wave(w).astype(np.float64) - ref).max())))
    return tuple(out)


@pytest.mark.parametrize("no_norm", [0, 1])
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("name", R.WAVE_CASES)
def test_wave_frames_equal_the_float64_statement(L, name, mode, no_norm):
    """Every element: |planes - frames64(wave_norm64(x))| <= 2 e_ref + u_mode |ref| (+ eta_mode, see unit_roundoff), e_ref the numpy
    fp32 oracle's distance from the statement on that clip.  With no_norm the rows are the samples themselves: the planes are the host
    split of them bit for bit.  Columns k .. 63 are zero, rows outside [0, total_rows) keep their canaries, the 64 (sum, sum^2) partials
    left in `work` (ser_gn_stats_v reads them) add up to the float64 sums, and the fp16 range guard stays clear."""
    clips = wave_reference(name)
    B = len(clips)
    lens = [len(w) for w, _, _ in clips]
    T = [R.n_frames(n, K, STRIDE) for n in lens]
    rows = sum(T)
    packed = torch.from_numpy(np.concatenate([w for w, _, _ in clips])).to(DEV)
    soffs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    foffs = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=DEV)
    P = 1 if mode == BF16 else 2
    all_rows = PRE + rows + POST
    buf = torch.full((P, all_rows, 64), FILL, dtype=torch.int16, device=DEV)
    ws = L.lib.ser_workspace_bytes(L.WS_WAVE_FRAMES, B, 0, 0, 0, mode)
    assert ws == B * 64 * 2 * 8
    work = torch.full((B * 64 * 2 + 16,), -7.0, dtype=torch.float64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.WaveFramesArgs()
    a.wav, a.sample_offs, a.frame_offs, a.B, a.k, a.stride, a.mode = packed.data_ptr(), soffs.data_ptr(), foffs.data_ptr(), B, K, STRIDE, mode
    a.out, a.out_plane_stride, a.work, a.total_rows, a.no_norm = buf.data_ptr() + PRE * 64 * 2, all_rows * 64, work.data_ptr(), rows, no_norm
    a.range_flag = flag.data_ptr()
    L.check(L.lib.ser_wave_frames_v(C.byref(a), stream()), "ser_wave_frames_v")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:, :PRE] == FILL).all()) and bool((host[:, PRE + rows:] == FILL).all()), "rows outside [0, total_rows) were written"
    words = host[:, PRE: PRE + rows]
    value = words.view(torch.float16 if mode == FP16X else torch.bfloat16).double().sum(0).numpy()          # [rows, 64]
    assert np.isfinite(value).all()
    assert not value[:, K:].any() and not bool(words[:, :, K:].any()), "columns k .. 63 must be zero words"
    assert int(flag.item()) == 0, "the fp16 range guard tripped on samples of magnitude <= 1"

    u, eta = unit_roundoff(mode)
    part = work.cpu().numpy()
    assert (part[B * 128:] == -7.0).all(), "ser_wave_frames_v wrote past its [B][64][2] partials"
    part = part[: B * 128].reshape(B, 64, 2)
    o = 0
    worst_err, worst_ratio, worst_eref = 0.0, 0.0, 0.0
    for b, (w, normed, e_ref) in enumerate(clips):
        x = w.astype(np.float64)
        # the partials: the same fp64 terms in another order
        assert abs(part[b, :, 0].sum() - x.sum()) <= 1e-12 * np.abs(x).sum(), (b, part[b, :, 0].sum(), x.sum())
        assert abs(part[b, :, 1].sum() - (x * x).sum()) <= 1e-12 * (x * x).sum(), (b, part[b, :, 1].sum(), (x * x).sum())
        if no_norm:
            ref, e_ref = R.frames64(x, K, STRIDE), 0.0
            assert torch.equal(words[:, o: o + T[b]], host_planes(torch.from_numpy(ref).float(), mode)), (b, "planes != host split")
        else:
            ref = R.frames64(normed, K, STRIDE)
            if name in ("constant 0.25", "zeros"):
                assert not bool(words[:, o: o + T[b]].any()), "a constant clip normalises to exactly 0"
        err = np.abs(value[o: o + T[b]] - ref)
        tol = 2.0 * e_ref + u * np.abs(ref) + eta
        worst_err, worst_eref = max(worst_err, float(err.max())), max(worst_eref, e_ref)
        worst_ratio = max(worst_ratio, float((err / tol).max()))
        assert (err <= tol).all(), (b, len(w), float(err.max()), float((err / tol).max()))
        o += T[b]
    assert o == rows
    record(f"wave_frames {name} {MODE_NAME[mode]} no_norm {no_norm}: kernel {worst_err:.3e} e_ref {worst_eref:.3e} "
           f"worst err / gate {worst_ratio:.3f} ({rows} rows)")
