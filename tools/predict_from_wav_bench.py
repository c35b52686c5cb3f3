"""What predictor.score_from_wav and its kernel cost, measured on the GPU; not a test.

1. Kernel: HIP-event medians of ser_select_rows_v gathering 16 x 500 and 16 x 1 280 rows of 1 280 columns out of 1 500-row windows (the
   Whisper-large-v3 crop), in f16x and bf16, set against ser_pack_rows_flagged over the same number of CONTIGUOUS rows -- the step it
   replaces in the heads, and the yardstick that exists without it.  Alternated twice in the same call.  Bytes: 4 M D read, 2 P M D written.
2. End to end: files per second of score_from_wav at Whisper-large-v3 + RoBERTa-large geometry with synthetic weights on ten-second wav
   files in a memory-backed directory, set against the route through feature files over the same corpus: driver.run_whisper,
   driver.run_roberta, head.score(engine="hip").  Alternated twice.  The synthetic weights are generated once and shared; every figure
   includes building its route's encoders from them, decoding, and writing results/test.csv.

    python tools/predict_from_wav_bench.py [--files 256] [--seconds 10] [--reps 50] [--mode f16mf] [--out profiles/predict_from_wav.txt]
                                           [--skip_kernel] [--skip_e2e]
"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from interspeech_ser_amd import _lib                                             # noqa: E402

DEV = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def event_times(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in evs])


def kernel_part(reps):
    B, W, D = 16, 1500, 1280
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=DEV).manual_seed(1)
    src = [torch.randn((B * W, D), device=DEV, generator=gen) for _ in range(4)]
    say(f"ser_select_rows_v against ser_pack_rows_flagged: B = {B} windows of {W} rows, D = {D}; HIP events, {reps} launches after 5 warm-up")
    for count in (500, 1280):
        M = B * count
        so = torch.tensor([b * W for b in range(B)], dtype=torch.int32, device=DEV)
        do = torch.tensor([b * count for b in range(B + 1)], dtype=torch.int32, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        for mode_name, mode, planes, dt in (("f16x", _lib.MODE_FP16X, 2, torch.float16), ("bf16", _lib.MODE_BF16, 1, torch.bfloat16)):
            out = torch.empty((planes, M, D), dtype=dt, device=DEV)

            def args(n_src):
                a = _lib.SelectRowsArgs()
                for k in range(n_src):
                    a.src[k] = src[k].data_ptr()
                a.ld_src, a.src_offs, a.dst_offs = D, so.data_ptr(), do.data_ptr()
                a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = out.data_ptr(), D, M * D, flag.data_ptr()
                a.n_src, a.B, a.D, a.max_rows, a.mode = n_src, B, D, count, mode
                return a
            a1, a4 = args(1), args(4)
            select = lambda: _lib.check(_lib.lib.ser_select_rows_v(C.byref(a1), st), "ser_select_rows_v")
            select4 = lambda: _lib.check(_lib.lib.ser_select_rows_v(C.byref(a4), st), "ser_select_rows_v")
            pack = lambda: _lib.check(_lib.lib.ser_pack_rows_flagged(src[0].data_ptr(), D, 1, M, D, 0, out.data_ptr(), D, M * D, mode,
                                                                     flag.data_ptr(), st), "ser_pack_rows_flagged")
            nbytes = 4 * M * D + 2 * planes * M * D
            for rnd in range(2):                           # alternated
                for name, fn, nb in (("ser_select_rows_v (1 source)", select, nbytes), ("ser_pack_rows_flagged (contiguous)", pack, nbytes),
                                     ("ser_select_rows_v (mean of 4)", select4, nbytes + 12 * M * D)):
                    t = event_times(fn, reps)
                    med = float(np.median(t))
                    say(f"   {B} x {count:4d} rows {mode_name:4s} round {rnd}: {name:36s} median {med:7.1f} us (min {t.min():7.1f})  "
                        f"{1e3 * med / M:6.2f} ns per row  {nb / 1e6:6.1f} MB  {nb / med / 1e3:7.1f} GB/s")
            assert int(flag.item()) == 0


def e2e_part(n_files, seconds, mode):
    import pandas as pd
    from interspeech_ser_amd import config as CF
    from interspeech_ser_amd import driver
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.predictor import score_from_wav
    from oracle.fusion_head import seeded_head_weights
    import fusion_ref as R
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="predict_from_wav_", dir=base)
    try:
        wav_dir = os.path.join(root, "Audios")
        os.makedirs(wav_dir)
        names = [f"MSP-PODCAST_{i:05d}.wav" for i in range(n_files)]
        rng = np.random.default_rng(0)
        n = int(16000 * seconds)
        t = np.arange(n) / 16000.0
        for name in names:
            x = 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * rng.uniform(100.0, 400.0) * t)
            with wave.open(os.path.join(wav_dir, name), "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
        words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
        texts = [" ".join(words[(i + j) % 8] for j in range(5 + i % 20)) for i in range(n_files)]
        pd.DataFrame({"FileName": names, "transcription": texts}).to_csv(os.path.join(root, "text.csv"), index=False)
        pd.DataFrame({"FileName": names}).to_csv(os.path.join(root, "test.csv"), index=False)
        geo_t = CF.ROBERTA_LARGE
        max_len = 80

        def tokenize(batch):                               # stand-in tokenizer: the hub's vocabulary is not needed for a timing
            ids = torch.full((len(batch), max_len), geo_t.pad_token_id, dtype=torch.int64)
            mask = torch.zeros((len(batch), max_len), dtype=torch.int64)
            for i, s in enumerate(batch):
                toks = ([0] + [3 + (len(w) * 7919 + j) % (geo_t.vocab_size - 4) for j, w in enumerate(s.split())])[: max_len - 1] + [2]
                ids[i, : len(toks)] = torch.tensor(toks)
                mask[i, : len(toks)] = 1
            return ids, mask

        sd = seeded_head_weights(R.head_shapes(1280, 1024), 31)
        cache, real = {}, driver.find_weights

        def cached_weights(name, *a, **k):
            if name not in cache:
                cache[name] = real(name, *a, **k)
            return cache[name]
        driver.find_weights = cached_weights
        wname, tname = "openai/whisper-large-v3", "roberta-large"
        say(f"score_from_wav against the route through feature files: {n_files} files of {seconds:g} s in {root}, {wname} ({mode}) + {tname} (f16x), "
            f"head f16x, batches of 16, synthetic weights generated once")

        def cfg(tag, rnd):
            c = {"wav_dir": wav_dir, "txt_dir": os.path.join(root, "text.csv"), "lazy_dir1": os.path.join(root, f"whisper_{rnd}"),
                 "lazy_dir2": os.path.join(root, f"roberta_{rnd}"), "feat1_dim": 1280, "feat2_dim": 1024, "model_path": os.path.join(root, f"exp_{tag}_{rnd}")}
            os.makedirs(c["model_path"])
            torch.save(sd, os.path.join(c["model_path"], "multimodal_ser.pt"))
            return c
        for rnd in range(2):                               # alternated
            c = cfg("files", rnd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            driver.run_whisper(["--ssl_type", wname, "--wav_dir", wav_dir, "--save_path", c["lazy_dir1"], "--synthetic_weights", "--mode", mode,
                                "--batch_size", "16"])
            t1 = time.perf_counter()
            driver.run_roberta(["--roberta_type", tname, "--df_path", c["txt_dir"], "--save_path", c["lazy_dir2"], "--synthetic_weights",
                                "--mode", "f16x", "--batch_size", "16", "--max_len", str(max_len)], tokenize=tokenize)
            t2 = time.perf_counter()
            ra = HD.score(c, engine="hip", mode="f16x", test_csv=os.path.join(root, "test.csv"))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            say(f"   round {rnd}: feature files: whisper driver {t1 - t0:6.2f} s, text driver {t2 - t1:6.2f} s, head.score {t3 - t2:6.2f} s, "
                f"together {t3 - t0:6.2f} s = {ra['n'] / (t3 - t0):7.1f} files/s ({ra['n']} rows, {ra['failed']} failed)")
            c = cfg("wav", rnd)
            t0 = time.perf_counter()
            rb = score_from_wav(c, [wname, tname], test_csv=os.path.join(root, "test.csv"), mode=mode, text_mode="f16x", head_mode="f16x",
                                batch_size=16, max_len=max_len, synthetic_weights=True, tokenize=tokenize)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            say(f"   round {rnd}: score_from_wav {t1 - t0:6.2f} s = {rb['n'] / (t1 - t0):7.1f} files/s ({rb['n']} rows, {rb['failed']} failed)")
            with open(ra["csv"], "rb") as fa, open(rb["csv"], "rb") as fb:
                say(f"   round {rnd}: the two results/test.csv are {'byte-identical' if fa.read() == fb.read() else 'DIFFERENT'}")
            for d in (c["lazy_dir1"], c["lazy_dir2"]):
                shutil.rmtree(d, ignore_errors=True)
        driver.find_weights = real
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--files", type=int, default=256)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--mode", type=str, default="f16mf")
    p.add_argument("--out", type=str, default="")
    p.add_argument("--skip_kernel", action="store_true")
    p.add_argument("--skip_e2e", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no MI355X visible: nothing is measured without one")
    if not a.skip_kernel:
        kernel_part(a.reps)
    if not a.skip_e2e:
        e2e_part(a.files, a.seconds, a.mode)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
