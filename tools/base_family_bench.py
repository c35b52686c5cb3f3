"""WavLM-base (GroupNorm stem, post-LN encoder) on the GPU box: 16 x 10 s, synthetic weights.

    python tools/base_family_bench.py [--modes f16x,bf16] [--iters 20] [--e2e 64]

Prints one JSON line per mode: forward utt/s (device events around replayed forwards, after warm-up), the conv stem's time
(launch by launch: ser_wave_frames -> ser_gn_stats -> conv 0..6; the same launches with the layer-norm stem of the same widths
for comparison), and the end-to-end driver rate on --e2e ragged 3-10 s files on tmpfs (wall clock around run_speech, weight generation
included; the driver's own SER_RUN line, printed above the JSON, gives the rate of the extraction loop alone).  The statistics kernels' own times come
from a separate ``rocprofv3 --kernel-trace --stats`` run of this script (gn_moments_kernel, gn_finalize_kernel)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave
from dataclasses import replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import config as C          # noqa: E402
from interspeech_ser_amd import driver               # noqa: E402
from interspeech_ser_amd.engine import SpeechEncoder  # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict  # noqa: E402


def stem_ms(enc, dev, lengths, iters):
    """mean time of the conv stem (framing, GN statistics / LN epilogues, conv 0..6), launched one by one"""
    pl = enc._plan(lengths, 0)
    enc.use_tape = False
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]

    def launches():                       # the stem only: _launches up to the feature projection
        enc._st = torch.cuda.current_stream().cuda_stream
        enc._guard_word(pl)
        try:
            enc.__class__._stem_only(enc, pl, dev)
        finally:
            enc._st = None
    for _ in range(3):
        launches()
    for e0, e1 in ev:
        e0.record()
        launches()
        e1.record()
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in ev]))


def _stem_only(self, pl, packed_wave):
    """conv layers 0..6 of SpeechEncoder._launches (ser_wave_frames, the stem's GEMMs); nothing after the last conv"""
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import Act
    import ctypes as Cc
    geo = self.geo
    a = _lib.WaveFramesArgs()
    fr = pl["frames"]
    a.wav, a.sample_offs, a.frame_offs = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["frame_offs0"].data_ptr()
    a.B, a.k, a.stride, a.mode = pl["B"], geo.conv_kernel[0], geo.conv_stride[0], self.stem_mode
    a.out, a.out_plane_stride, a.work, a.total_rows = fr.ptr, fr.plane_stride, pl["wave_work"].data_ptr(), pl["rows"][0]
    a.range_flag = self._flag
    _lib.check(_lib.lib.ser_wave_frames_v(Cc.byref(a), self._s()), "ser_wave_frames")
    a_in = pl["conv_act"][0]
    if self.post_ln:
        self._groupnorm_stem(pl, packed_wave)
    else:
        self._gemm(fr, self.conv0, pl["rows"][0], act=_lib.ACT_GELU, ln=self.conv_ln[0], ln_eps=1e-5, out_act=a_in, stem=True)
    nl, C0 = len(geo.conv_dim), geo.conv_dim[0]
    for i in range(1, nl):
        rows = pl["rows"][i]
        if i < nl - 1:
            a_out = pl["conv_act"][i % 2]
            v = Act.__new__(Act)
            v.t, v.rows, v.cols, v.planes, v.plane_stride = a_out.t, rows, C0, a_out.planes, a_out.plane_stride
            self._gemm(a_in, self.convs[i - 1], rows, a_rowoff=pl["conv_rowoff"][i - 1], act=_lib.ACT_GELU, ln=self.conv_ln[i],
                       ln_eps=1e-5, out_act=v, stem=True)
            a_in = v
        else:
            self._gemm(a_in, self.convs[i - 1], rows, a_rowoff=pl["conv_rowoff"][i - 1], act=_lib.ACT_GELU, ln=self.conv_ln[i],
                       ln_eps=1e-5, out_f32=pl["feat_f32"], ldo_f32=C0, stem=True)


SpeechEncoder._stem_only = _stem_only


def forward_rate(enc, dev, lengths, iters):
    enc.use_tape = True
    for _ in range(3):
        enc.forward(dev, lengths)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        enc.forward(dev, lengths)
    e1.record()
    torch.cuda.synchronize()
    return len(lengths) * iters / (e0.elapsed_time(e1) / 1e3)


def e2e_rate(n, mode):
    root = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    wav_dir, out = os.path.join(root, "wav"), os.path.join(root, "pt")
    os.makedirs(wav_dir)
    rng = np.random.default_rng(4321)
    for i in range(n):
        L = int(rng.uniform(3.0, 10.0) * 16000)
        pcm = (np.clip(0.1 * rng.standard_normal(L), -1, 1) * 32767).astype("<i2")
        with wave.open(os.path.join(wav_dir, f"syn_{i:05d}.wav"), "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    t0 = time.perf_counter()
    driver.run_speech(["--ssl_type", "microsoft/wavlm-base", "--wav_dir", wav_dir, "--save_path", out, "--synthetic_weights",
                       "--use_n_layer", "--n_layer", "-1", "--mode", mode, "--batch_size", "16"])
    dt = time.perf_counter() - t0
    done = len(os.listdir(out))
    shutil.rmtree(root)
    return done / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f16x,bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=64)
    args = ap.parse_args()
    geo = C.WAVLM_BASE
    sd = synthetic_state_dict(geo, 7, fast=True)
    # the layer-norm stem of the same conv widths: the stable-LN form of the same geometry (its LN keys added)
    geo_ln = replace(geo, feat_extract_norm="layer", stable_layer_norm=True, name="wavlm-base-as-layer-norm-stem")
    sd_ln = synthetic_state_dict(geo_ln, 7, fast=True)
    rng = np.random.default_rng(0)
    waves = [(0.1 * rng.standard_normal(160000)).astype(np.float32) for _ in range(16)]
    lengths = [len(w) for w in waves]
    for mode in args.modes.split(","):
        enc = SpeechEncoder(geo, sd, "cuda:0", mode=mode)
        dev = enc.upload(waves)
        fwd = forward_rate(enc, dev, lengths, args.iters)
        gn_ms = stem_ms(enc, dev, lengths, args.iters)
        del enc
        enc_ln = SpeechEncoder(geo_ln, sd_ln, "cuda:0", mode=mode)
        ln_ms = stem_ms(enc_ln, enc_ln.upload(waves), lengths, args.iters)
        del enc_ln
        torch.cuda.empty_cache()
        e2e = e2e_rate(args.e2e, mode) if args.e2e else None
        print(json.dumps({"model": geo.name, "mode": mode, "batch": "16 x 10 s", "forward_utt_per_s": round(fwd, 1),
                          "stem_ms_groupnorm": round(gn_ms, 3), "stem_ms_layernorm_same_widths": round(ln_ms, 3),
                          "e2e_driver_utt_per_s_incl_weight_init": None if e2e is None else round(e2e, 1)}), flush=True)


if __name__ == "__main__":
    main()
