"""End-to-end rate of the baseline prediction driver against the extraction driver on the same files: N synthetic 10 s wav files on
tmpfs, WavLM-large with synthetic weights, the two drivers alternated, two runs each per mode.  Extraction writes hidden_states[-1]
as .pt files to tmpfs (2 MB per utterance off the device); prediction brings 8 floats per utterance back and writes one CSV.

    python tools/pool_head_e2e.py [N, default 512] [modes, default bf16,f16mf] [output file]
"""
import contextlib
import io
import json
import os
import re
import shutil
import sys
import tempfile
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import baseline, driver          # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
modes = (sys.argv[2] if len(sys.argv) > 2 else "bf16,f16mf").split(",")
out_path = sys.argv[3] if len(sys.argv) > 3 else ""
root = tempfile.mkdtemp(dir="/dev/shm")
lines = []
try:                                     # the corpus (~160 MB at N = 512) leaves tmpfs however the run ends
    wav_dir, model = os.path.join(root, "wav"), os.path.join(root, "model")
    os.makedirs(wav_dir)
    os.makedirs(model)
    rng = np.random.default_rng(4321)
    for i in range(n):
        pcm = (np.clip(0.1 * rng.standard_normal(160000), -1, 1) * 32767).astype("<i2")
        with wave.open(os.path.join(wav_dir, f"syn_test3_{i:05d}.wav"), "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    cfg = os.path.join(root, "config.json")
    with open(cfg, "w") as f:
        json.dump({"wav_dir": wav_dir, "label_path": ""}, f)


    def rate(fn, argv):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fn(argv)
        m = re.search(r"(\d+) utterances on 1 GPU\(s\) in ([0-9.]+) s \(([0-9.]+) utt/s\)", buf.getvalue())
        if not m:
            print(buf.getvalue())
            raise SystemExit("no rate line")
        return int(m.group(1)), float(m.group(3))


    lines.append(f"{n} synthetic 10 s files on tmpfs, WavLM-large (synthetic weights), batch 16, 4 workers; loop time only (weights loaded before)")
    for mode in modes:
        for run in (1, 2):
            pt = os.path.join(root, f"pt_{mode}_{run}")
            done, r = rate(driver.run_speech, ["--ssl_type", "microsoft/wavlm-large", "--wav_dir", wav_dir, "--save_path", pt, "--synthetic_weights",
                                               "--use_n_layer", "--n_layer", "-1", "--mode", mode])
            lines.append(f"mode {mode} run {run}: extraction (hidden_states[-1] -> .pt)  {done} files  {r:8.1f} utt/s")
            shutil.rmtree(pt)
            done, r = rate(baseline.run_eval_cat, ["--ssl_type", "wavlm-large", "--model_path", model, "--config_path", cfg, "--synthetic_weights",
                                                   "--mode", mode])
            lines.append(f"mode {mode} run {run}: prediction (pooling + head -> CSV)      {done} files  {r:8.1f} utt/s")
finally:
    shutil.rmtree(root, ignore_errors=True)
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a") as f:
        f.write(text + "\n")
