"""Times the CTC head and the transcription command (GPU; profiles/ctc.txt quotes this tool's output).

Part 1, the head's launches.  engine.CTCHead behind a speech encoder of width D = 1024 (wavlm-large geometry) and D = 1280
(hubert-xlarge), V = 32, on the rows of 16 x 10 s (M = 7 984) of seeded hidden states, modes f16x and bf16: WARMUP warm-up calls, then
REPEATS traced calls (one HIP event pair per step: the operand copy, the lm_head ser_gemm, ser_ctc_greedy_v's two kernels); median, min
and max over the repeats.  The logits are M x 32 x 4 B = 1 MB.

Part 2, files/s.  N_FILES seeded ten-second wav files on local disk, hubert-xlarge geometry with seeded weights (no published checkpoint is
available offline), batches of 16: ctc.run (preprocessing/transcribe_ctc.py's function, the model handed in ready-made, so weight loading
is outside the timed loop) against driver._run (preprocessing/preprocess_speech.py's function, --use_n_layer --n_layer -1: the full
forward, the last state written per file), the same files, the same mode, alternated, one untimed pass each first and then two timed
passes each; the figure is each command's own "utterances ... utt/s" line, which covers its loop (decode, upload, forward, copy back,
write) and not the model's construction.

    python tools/ctc_bench.py [out.txt] [n_files]
"""
from __future__ import annotations

import contextlib
import io
import os
import re
import shutil
import sys
import tempfile
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                     # noqa: E402

WARMUP, REPEATS, BATCH, SECONDS, V = 3, 20, 16, 10, 32
N_FILES = 256


def synthetic_lm_head(D: int, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {"lm_head.weight": torch.randn(V, D, generator=g) * 0.05, "lm_head.bias": torch.randn(V, generator=g) * 0.5}


def head_times(lines, geo, mode: str) -> None:
    from interspeech_ser_amd.engine import CTCHead, HiddenStates, build_encoder
    enc = build_encoder(geo, synthetic_state_dict(geo, 7, fast=True), "cuda:0", mode)
    head = CTCHead(enc, synthetic_lm_head(geo.hidden, 3), C.CTCSpec(V, 0, "HubertForCTC"))
    T = geo.frames_for(SECONDS * 16000)
    offs = [b * T for b in range(BATCH + 1)]
    g = torch.Generator(device="cuda").manual_seed(5)
    states = torch.randn((1, offs[-1], geo.hidden), generator=g, device="cuda", dtype=torch.float32)
    hs = HiddenStates(states, offs)
    steps = {}
    for it in range(WARMUP + REPEATS):
        head.trace = [] if it >= WARMUP else None
        head.forward_tokens(hs)
        torch.cuda.synchronize()
        if head.trace is not None:
            for n, a, b in head.trace:
                steps.setdefault(n, []).append(1e3 * a.elapsed_time(b))
    head.trace = None
    assert head.status() == 0
    fmt = lambda v: f"median {np.median(v):.1f} min {min(v):.1f} max {max(v):.1f}"      # noqa: E731
    lines.append(f"D = {geo.hidden} ({geo.name}), M = {offs[-1]}, V = {V}, mode {mode}; us per call over {REPEATS} traced calls: "
                 + "; ".join(f"{n} {fmt(v)}" for n, v in steps.items()))
    del enc, head
    torch.cuda.empty_cache()


def write_wavs(path: str, n: int) -> None:
    rng = np.random.default_rng(0)
    t = np.arange(SECONDS * 16000) / 16000.0
    for i in range(n):
        x = 0.1 * rng.standard_normal(t.size) + 0.2 * np.sin(2 * np.pi * (110.0 + 7 * (i % 40)) * t)
        with wave.open(os.path.join(path, f"syn_{i:05d}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2").tobytes())


def rate_of(text: str) -> float:
    m = re.findall(r"utterances on 1 GPU\(s\) in [0-9.]+ s \(([0-9.]+) utt/s\)", text)
    if not m:
        raise SystemExit("no utt/s line in:\n" + text[-2000:])
    return float(m[-1])


def files_per_second(lines, mode: str, n_files: int) -> None:
    from interspeech_ser_amd import ctc as CT
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.engine import build_encoder
    geo = C.geometry_for("facebook/hubert-xlarge-ls960-ft")
    sd = synthetic_state_dict(geo, 7, fast=True)
    full = dict(sd)
    full.update(synthetic_lm_head(geo.hidden, 3))
    tr = CT.CTCTranscriber(geo, C.CTCSpec(V, 0, "HubertForCTC"), full, "cuda:0", mode)
    tr.weight_source = "seeded weights"
    enc = build_encoder(geo, sd, "cuda:0", mode)
    del sd, full
    tmp = tempfile.mkdtemp(prefix="ctc_bench_")
    try:
        wav_dir = os.path.join(tmp, "wavs")
        os.makedirs(wav_dir)
        write_wavs(wav_dir, n_files)

        def transcribe():
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                CT.run(["--model", geo.name, "--wav_dir", wav_dir, "--out_csv", os.path.join(tmp, "t.csv"), "--mode", mode],
                       transcriber_factory=lambda a, d: tr, vocab=None)
            assert f"Wrote {n_files} of {n_files}" in buf.getvalue(), buf.getvalue()[-2000:]
            return rate_of(buf.getvalue())

        def extract():
            save = os.path.join(tmp, "feats")
            shutil.rmtree(save, ignore_errors=True)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                driver._run(["--ssl_type", geo.name, "--wav_dir", wav_dir, "--save_path", save, "--mode", mode, "--use_n_layer", "--n_layer", "-1",
                             "--synthetic_weights"], False, extractor_factory=lambda a, w, d: driver._Extractor.from_encoder(a, enc, w, "seeded weights"),
                            local_only=True)
            assert len(os.listdir(save)) == n_files, buf.getvalue()[-2000:]
            return rate_of(buf.getvalue())

        transcribe()
        extract()
        t, e = [], []
        for _ in range(2):
            e.append(extract())
            t.append(transcribe())
        lines.append(f"files/s, hubert-xlarge geometry, {n_files} x {SECONDS} s wav files, batches of 16, mode {mode} (alternated, every run): "
                     f"preprocess_speech {e[0]:.1f}, {e[1]:.1f}; transcribe_ctc {t[0]:.1f}, {t[1]:.1f}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    del tr, enc
    torch.cuda.empty_cache()


def main(out_path: str = "", n_files: int = N_FILES) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("ctc_bench needs the GPU: a CPU run measures nothing")
    lines = [f"CTC head: {BATCH} x {SECONDS} s, seeded weights, HIP events, {WARMUP} warm-up + {REPEATS} traced calls, one process"]

    def flush():
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    for geo in (C.geometry_for("microsoft/wavlm-large"), C.geometry_for("facebook/hubert-xlarge-ls960-ft")):
        for mode in ("f16x", "bf16"):
            head_times(lines, geo, mode)
            print(lines[-1], flush=True)
            flush()
    for mode in ("f16x", "bf16"):
        files_per_second(lines, mode, n_files)
        print(lines[-1], flush=True)
        flush()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else N_FILES)
