#!/usr/bin/env python
"""Headline benchmark: utterances/s of WavLM-large embedding extraction (10 s @ 16 kHz).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = one pass of the hot path (waveform normalisation -> conv stack -> projection ->
positional conv -> 24 encoder layers -> final LayerNorm, all L+1 hidden states written to HBM)
over one batch of 16 synthetic 10 s clips already resident in HBM (BASELINE.json configs[1]).
Utterances shard across ranks with no data-path collective (weak scaling): the only RCCL
traffic is the one-time broadcast of the frozen weights from rank 0.

A counted step covers `--reps` such batches (default 8, stated in `config`), so that the timed region of the default run
lasts > 1 s and a GPU-busy sampler can see it; `value` counts every utterance.  Round 3: `--inflight` whole batches (default 2)
run at once on parallel branches of one hipGraph, as the drivers' two-slot pipeline does with real files.

One JSON line on rank 0: metric/value/unit/dtype/ms_per_step and the workload's configuration.  A plain run does
nothing else: it sets up, warms up, times the steps, dumps (--dump-outputs) and prints.  `--full` adds, after the
timed region, `roofline` (dominant kernel = the MFMA GEMM, live HIP-event timing) + `verified` / `verification` (the
outputs of the very graph that was timed: bit-equal to the eager command-list path, within the timed mode's bound of
the CPU oracle) + `parity_mode*` (throughput and measured error of each numerics mode against north_star's 1e-3)
+ `end_to_end` (wav files on tmpfs -> decode -> H2D -> forward -> D2H -> .pt files through the driver)
+ `other_encoders` + `cpu_baseline` (CPU oracle, reference-style batch-of-one driver, bounded sample, rank 0 at N=1
only); the --no-* options drop single legs of such a run.
`ms_per_step` is the wall time of one counted step.

`--dump-outputs DIR` writes what the last timed step computed (a fixed sample of its hidden states, float32 .npy) to DIR
right after the timed region; the inputs and weights are seeded, so two builds run with the same arguments can be compared
output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"
DRIVER_DEFAULT_MODE = "f16mf"      # interspeech_ser_amd/driver.py --mode default
# BASELINE.json configs[2..4]'s encoders on their own batch shapes: (hub id, batch, seconds per clip)
OTHER_ENCODERS = {"xlsr": ("facebook/wav2vec2-xls-r-2b", 8, 10.0), "hubert": ("facebook/hubert-xlarge-ll60k", 16, 10.0),
                  "whisper": ("openai/whisper-large-v3", 16, 30.0)}


def algorithmic_gflop_per_utt(geo, num_samples):
    """2*MAC over valid frames only (384.0 for WavLM-large @ 10 s)."""
    chain = geo.frame_chain(num_samples)
    cin, fl = 1, 0.0
    for t, c, k in zip(chain, geo.conv_dim, geo.conv_kernel):
        fl += 2.0 * t * c * cin * k
        cin = c
    T, D, F, H = chain[-1], geo.hidden, geo.ffn, geo.heads
    fl += 2.0 * T * cin * D
    fl += 2.0 * T * D * (D // geo.pos_conv_groups) * geo.pos_conv_kernel
    per_layer = 2.0 * T * D * 3 * D + 2.0 * T * D * D + 2 * (2.0 * T * T * D) + 2 * (2.0 * T * D * F)
    return (fl + geo.num_layers * per_layer) / 1e9


def whisper_gflop_per_utt(geo):
    """Whisper encoder on the fixed 30 s window: stem convs + L pre-LN layers (2273.9 GF for large-v3)."""
    T, D, F = geo.max_source_positions, geo.hidden, geo.ffn
    stem = 2.0 * 3000 * D * geo.n_mels * 3 + 2.0 * T * D * D * 3
    per_layer = 2.0 * T * D * 3 * D + 2.0 * T * D * D + 2 * (2.0 * T * T * D) + 2 * (2.0 * T * D * F)
    return (stem + geo.num_layers * per_layer) / 1e9


def synth_batch(batch, num_samples, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.1 * torch.randn(num_samples, generator=g)).numpy() for _ in range(batch)]


def broadcast_weights(geo, seed, rank, fast=False):
    """C1: rank 0 owns the frozen weights; everyone else receives them over RCCL/xGMI in one
    flat fp32 bucket (interspeech_ser_amd/dist.py).  Returns (state dict, seconds, bytes)."""
    from interspeech_ser_amd import dist as D
    from interspeech_ser_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(geo, seed, fast=fast) if rank == 0 else None
    sd, dt, nbytes = D.broadcast_state_dict(sd)
    return sd, dt, nbytes


def collective_record(world, seconds, nbytes):
    """What the one collective of the job did, as the process group itself reports it: a SCALE record can then show that RCCL really
    carried the weights to N ranks (backend name and world size from torch.distributed, not from the command line)."""
    import torch.distributed as dist
    if world <= 1 or not dist.is_initialized():
        return {"backend": None, "ranks": 1, "bytes": 0, "seconds": 0.0, "GB_per_s": None, "what": "single process: no collective runs"}
    backend = dist.get_backend()
    return {"backend": ("nccl (= RCCL on ROCm)" if backend == "nccl" else backend), "ranks": dist.get_world_size(), "bytes": int(nbytes),
            "seconds": round(seconds, 4), "GB_per_s": round(nbytes / max(seconds, 1e-9) / 1e9, 2),
            "what": "one flat fp32 broadcast of the frozen weights from rank 0 (dist.broadcast_state_dict); no data-path collective"}


def other_encoder_run(name, device, mode, steps=3, warmup=1, parity_modes=("f16mf", "f16x", "f16m")):
    """A short, checked run of one of the other encoders BASELINE.json's configs name, so that the driver's record carries a timed line
    for them too (round-3 verdict, weak #13): seeded synthetic weights (fast generator), the launch shape the drivers use for that
    family, `steps` counted steps of >= 0.3 s; the replayed graph's states must equal the eager path bit for bit.  Round 5 (verdict r4
    #5): the same for the tolerance-grade modes -- the drivers' default f16mf, f16x and the faster f16m -- each with its worst-state error
    against the CPU oracle on utterance 0 (full geometry), under ``modes``."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import build_encoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    ssl_type, batch, seconds = OTHER_ENCODERS[name]
    t_all = time.perf_counter()
    geo = C.geometry_for(ssl_type)
    whisper = geo.family == C.FAMILY_WHISPER
    sd = synthetic_state_dict(geo, 0, fast=True)
    num_samples = int(round(seconds * 16000))
    inflight, micro = (1, 2) if whisper else (2, 1)
    cuts = [round(i * batch / micro) for i in range(micro + 1)]
    waves = [synth_batch(batch, num_samples, 4242 + j) for j in range(inflight)]
    lengths = [num_samples] * batch
    gf = whisper_gflop_per_utt(geo) if whisper else algorithmic_gflop_per_utt(geo, num_samples)
    ref = None

    def one_mode(m, with_error):
        nonlocal ref
        enc = build_encoder(geo, sd, device, m)
        groups = [(enc.upload(waves[j][a:b], slot=slot), lengths[a:b])
                  for slot, (j, a, b) in enumerate((j, a, b) for j in range(inflight) for a, b in zip(cuts[:-1], cuts[1:]))]
        torch.cuda.synchronize()
        graph, hs = enc.capture_concurrent(groups)
        for _ in range(warmup):
            graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graph.replay()
        torch.cuda.synchronize()
        reps = max(1, int(0.3 / max(time.perf_counter() - t0, 1e-4) / steps) + 1)
        t0 = time.perf_counter()
        for _ in range(steps * reps):
            graph.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kept = [h.states.clone() for h in hs]
        eager = [enc.forward(w, l, slot=slot) for slot, (w, l) in enumerate(groups)]
        torch.cuda.synchronize()
        same = all(torch.equal(k, e.states) for k, e in zip(kept, eager))
        finite = all(bool(torch.isfinite(k).all()) for k in kept)
        utts = batch * inflight * steps * reps
        r = {"mode": m, "value": round(utts / dt, 1), "unit": "utterances/s", "steps": steps, "batches_per_step": reps * inflight,
             "ms_per_batch": round(1e3 * dt / steps / reps / inflight, 3),
             "achieved_tflops_whole_path": round(utts / dt * gf / 1e3, 1), "frac_of_bf16_peak": round(utts / dt * gf / 1e3 / MFMA_BF16_PEAK_TFLOPS, 4),
             "verified": bool(same and finite), "graph_replay_equals_eager_bitwise": bool(same), "all_finite": finite}
        if with_error:
            if ref is None:
                ref = oracle_states(geo, sd, waves[0][0], whisper)        # CPU oracle, utterance 0, all states (checker only)
            rows = ref[0].shape[0]
            err = max(rel_err(eager[0].utterance(0, l).cpu()[:rows], x) for l, x in enumerate(ref))
            r.update({"max_rel_err_vs_oracle": float(f"{err:.3e}"), "tolerance": 1e-3, "within_tolerance": bool(err <= 1e-3)})
            r["verified"] = bool(r["verified"] and err <= 1e-3)
        del enc, hs, kept, eager, graph, groups
        torch.cuda.empty_cache()
        return r

    timed = one_mode(mode, with_error=False)
    rec = {"workload": f"{geo.name} embed extract, batch={batch} x {seconds:.0f} s, mode={mode}, {inflight} batch(es) in flight x {micro} group(s)",
           "gflop_per_utt": round(gf, 1)}
    rec.update({k: v for k, v in timed.items() if k != "mode"})
    rec["modes"] = {m: one_mode(m, with_error=True) for m in parity_modes if m != mode}
    rec["verified"] = bool(rec["verified"] and all(v["verified"] for v in rec["modes"].values()))
    rec["weights"] = "seeded synthetic (fast generator); errors: worst hidden state of utterance 0 against the fp32 CPU oracle"
    del sd
    rec["seconds_incl_weight_generation"] = round(time.perf_counter() - t_all, 1)
    return rec


def cpu_baseline(geo, sd, num_samples, n_clips=8):
    """The CPU oracle driven like the reference: batch of one, ThreadPoolExecutor(4)
    (preprocess_speech.py:120-122), default torch intra-op threads."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import ssl_oracle as O
    clips = synth_batch(n_clips + 1, num_samples, 4321)

    def one(w):
        with torch.no_grad():
            return O.speech_hidden_states(geo, sd, torch.from_numpy(O.zero_mean_unit_var(w)))[-1].shape

    one(clips[0])                                    # warm-up
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(one, clips[1:]))
    dt = time.perf_counter() - t0
    return {"value": round(n_clips / dt, 4), "unit": "utterances/s", "cores": int(torch.get_num_threads()),
            "kind": "port", "host_cpus": os.cpu_count(),
            "sample": f"{n_clips} x {num_samples / 16000:.0f} s clips, batch of 1, 4-thread driver, fp32 PyTorch-CPU oracle"}


def bench_text(args, geo, rank, world, device, D):
    """Next row 8f-1: RoBERTa text extraction, `--batch` texts of `--max_len` tokens per step (synthetic ids)."""
    from interspeech_ser_amd.engine import build_encoder
    sd, bcast_s, _ = broadcast_weights(geo, 0, rank)
    enc = build_encoder(geo, sd, device, args.mode)
    T = args.max_len
    g = torch.Generator().manual_seed(99 + rank)
    lens = torch.randint(8, T + 1, (args.batch,), generator=g)
    ids = torch.randint(3, geo.vocab_size, (args.batch, T), generator=g)
    ids[torch.arange(T)[None, :] >= lens[:, None]] = geo.pad_token_id
    ids_d, kl_d = ids.to(device=device, dtype=torch.int32), lens.to(device=device, dtype=torch.int32)
    # like the speech step: the batch runs as `micro` groups of texts on parallel branches of one hipGraph
    micro = (args.micro if args.micro > 0 else 2)                  # default: two groups of texts
    micro = micro if 1 < micro <= args.batch else 1
    cuts = [round(i * args.batch / micro) for i in range(micro + 1)]
    parts = [(ids_d[a:b].contiguous(), kl_d[a:b].contiguous()) for a, b in zip(cuts[:-1], cuts[1:])]
    for slot, (i_, k_) in enumerate(parts):
        enc.forward_device(i_, k_, slot=slot)
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(device=device) for _ in parts[1:]]
    graph = torch.cuda.CUDAGraph()
    hs = [None] * len(parts)                                       # the HiddenStates every replay writes, one per group
    with torch.cuda.graph(graph):
        main_stream = torch.cuda.current_stream()
        for st in sides:
            st.wait_stream(main_stream)
        for slot, st in enumerate(sides, start=1):
            with torch.cuda.stream(st):
                hs[slot] = enc.forward_device(*parts[slot], slot=slot)
        hs[0] = enc.forward_device(*parts[0], slot=0)
        for st in sides:
            main_stream.wait_stream(st)
    for _ in range(args.warmup):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        graph.replay()
    torch.cuda.synchronize()
    elapsed = D.max_over_ranks(time.perf_counter() - t0)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, hs)
    if rank == 0:
        Dm, F, L = geo.hidden, geo.ffn, geo.num_layers
        gf = L * (2.0 * T * Dm * 3 * Dm + 2.0 * T * Dm * Dm + 4.0 * T * T * Dm + 4.0 * T * Dm * F) / 1e9
        value = args.batch * args.steps * world / elapsed
        print(json.dumps({"metric": f"texts/sec ({T} tokens) {geo.name} embed extract", "value": round(value, 1),
                          "unit": "texts/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "bf16" if args.mode == "bf16" else "bf16x3 (fp32-grade split)",
                          "data": "synthetic", "config": {"workload": f"{geo.name} text embed extract, batch={args.batch} x {T} tokens, mode={args.mode}, {micro} concurrent group(s)",
                                                          "gflop_per_text": round(gf, 1)},
                          "achieved_tflops_whole_path": round(value * gf / 1e3 / world, 1)}), flush=True)
    D.shutdown()


def kernel_source_digest():
    """sha256 over the kernel sources: a PMC summary under profiles/ is only quoted when it was taken from these kernels."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(ROOT, "interspeech_ser_amd", "csrc")
    files = sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith((".hip", ".h")))
    for f in files + [os.path.join(ROOT, "include", "ser_hip.h")]:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def dump_outputs(out_dir, hs_list, budget=48 << 20):
    """--dump-outputs: what a caller of the timed path receives from its last step -- hidden states 0..L of every utterance
    of every group -- as .npy files.  All of it is 1.6 GB at the headline shape, so at most `budget` bytes of (utterance, frame)
    rows are kept, drawn with a fixed seed from the output's shape alone: two builds run with the same arguments dump the same rows.
      hidden_states.npy  float32 [L+1, R, D]: the sampled rows of every state
      rows.npy           float64 [R, 3]: (group, utterance in the group, frame) of each sampled row"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    index = np.array([(g, u, t) for g, h in enumerate(hs_list) for u in range(h.batch) for t in range(h.frames(u))], dtype=np.int64)
    n_states, dim = min(h.computed for h in hs_list), hs_list[0].states.shape[-1]
    keep = min(len(index), budget // (4 * n_states * dim))
    rows = index[np.sort(np.random.default_rng(0).choice(len(index), size=keep, replace=False))]    # (g, u, t) order = group order
    parts = []
    for g, h in enumerate(hs_list):
        sel = [h.frame_offs[u] + t for _, u, t in rows[rows[:, 0] == g]]
        parts.append(h.states[:n_states].index_select(1, torch.tensor(sel, dtype=torch.long, device=h.states.device)).float().cpu())
    np.save(os.path.join(out_dir, "hidden_states.npy"), torch.cat(parts, 1).numpy())
    np.save(os.path.join(out_dir, "rows.npy"), rows.astype(np.float64))


def rel_err(got, ref):
    """max|a-b| / max(1, max|b|): the tolerance form of tests/test_gpu_e2e.py."""
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


def states_err(hs_a, ua, hs_b, ub):
    """worst rel_err over all L+1 states of utterance ua of hs_a against utterance ub of hs_b (same length)."""
    return max(rel_err(hs_a.utterance(ua, l).float(), hs_b.utterance(ub, l).float()) for l in range(len(hs_a)))


def oracle_states(geo, sd, wave, whisper):
    from oracle import ssl_oracle as O                    # checker only
    with torch.no_grad():
        if whisper:
            return O.whisper_hidden_states(geo, sd, torch.from_numpy(O.whisper_log_mel(wave, geo.n_mels)))
        return O.speech_hidden_states(geo, sd, torch.from_numpy(O.zero_mean_unit_var(wave)))


def end_to_end_leg(args, enc, geo, whisper, n_files, num_samples, world=1, D=None, mode=None, passes=3, with_ref_rule=True):
    """SURVEY 8d timing (ii): wav files on tmpfs -> decode -> pinned H2D -> forward -> selection -> D2H -> .pt on tmpfs,
    through the product's own driver (preprocess_speech.py:47-71 per file), re-using the encoder that was just timed.
    At N > 1 every rank runs the leg on its own directory of n files (weak scaling, like the headline): the record is
    sum(utterances) / max(wall) over the ranks -- what host-side decode / write contention between the ranks leaves."""
    import shutil
    import tempfile
    import wave as wavmod
    import numpy as np
    from interspeech_ser_amd import driver
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="ser_e2e_", dir=base)
    try:
        wav_dir = os.path.join(root, "wav")
        os.makedirs(wav_dir)
        # bound the leg by what the tmpfs can hold: a pass keeps n wav files (2 bytes / sample) plus its n outputs ([T, D] fp32)
        out_bytes = 4.0 * geo.hidden * (min(-(-num_samples // 320), geo.hidden) if whisper else geo.frames_for(num_samples))
        free = shutil.disk_usage(root).free
        n_files = int(max(args.batch * 4, min(n_files, 0.4 * free / world / (2.0 * num_samples + out_bytes))))
        rng = np.random.default_rng(4321)
        clips = [(np.clip(0.1 * rng.standard_normal(num_samples), -1, 1) * 32767).astype("<i2").tobytes() for _ in range(64)]
        for i in range(n_files):                                  # 64 distinct clips under n names: the driver cannot tell
            with wavmod.open(os.path.join(wav_dir, f"syn_{i:05d}.wav"), "wb") as wf:
                wf.setnchannels(1)
                wf.setsampwidth(2)
                wf.setframerate(16000)
                wf.writeframes(clips[i % 64])
        factory = lambda a, w, d: driver._Extractor.from_encoder(a, enc, w)          # noqa: E731
        import contextlib
        import io
        sink = io.StringIO()
        # two passes over the same files: the first grows the encoder's per-slot arenas from the 8-utterance groups of the timed
        # region to whole batches and records their command lists (one-time work of a long-running extraction); the second is reported
        def one_pass(tag, extra):
            out_dir = os.path.join(root, "pt_" + tag)
            argv = ["--ssl_type", args.ssl_type, "--wav_dir", wav_dir, "--save_path", out_dir, "--mode", mode or args.mode,
                    "--batch_size", str(args.batch), "--num_workers", str(args.e2e_workers)] + extra
            driver.LAST_RUN.clear()
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(io.StringIO()):
                (driver.run_whisper if whisper else driver.run_speech)(argv, extractor_factory=factory, local_only=True)
            res = dict(driver.LAST_RUN) or None
            if world > 1:                                         # whole-job figures: every rank's files over the slowest rank's wall
                done, wall = D.sum_over_ranks(res["done"] if res else 0), D.max_over_ranks(res["wall_s"] if res else 0.0)
                if res:
                    res["done"], res["wall_s"] = done, wall
            n_out = len(os.listdir(out_dir)) if os.path.isdir(out_dir) else 0
            shutil.rmtree(out_dir, ignore_errors=True)
            return res, n_out

        # the LAST hidden state (every layer runs): --use_n_layer --n_layer -1.  Three timed passes after the warm one.
        full = ["--use_n_layer", "--n_layer", "-1"]
        one_pass("warm", full)
        runs = [one_pass(f"timed{i}", full) for i in range(passes)]
        # the reference's own default on a fresh directory: hidden_states[0] (preprocess_speech.py:41,67), where the forward stops
        # after the positional conv (driver: last_state) -- the speech script's README recipe
        ref_rule = None
        if not whisper and with_ref_rule:
            one_pass("warm0", [])
            r0, n0 = one_pass("rule0", [])
            if r0 and n0 == n_files:
                ref_rule = {"value": round(r0["done"] / r0["wall_s"], 1), "unit": "utterances/s", "wall_s": round(r0["wall_s"], 3),
                            "what": "same files, the reference's default layer rule on a fresh --save_path: hidden_states[0], "
                                    "encoder layers not launched (early exit)"}
        ok = [(r, n) for r, n in runs if r and n == n_files]
        last, written = (sorted(ok, key=lambda rn: rn[0]["done"] / rn[0]["wall_s"])[len(ok) // 2] if ok else (None, 0))
        if not last or written != n_files:
            return {"error": f"driver wrote {written} of {n_files} files", "log_tail": sink.getvalue()[-400:]}
        if world > 1:
            n_files *= world
        t = last["launch_thread"]
        rates = sorted(r["done"] / r["wall_s"] for r, _ in ok)
        rec = {"value": round(last["done"] / last["wall_s"], 1), "unit": "utterances/s", "mode": mode or args.mode, "files": n_files, "n_gpus": world,
               "wall_s": round(last["wall_s"], 3), "batch_size": args.batch, "host_threads": args.e2e_workers,
               "passes": len(ok), "min": round(rates[0], 1), "median": round(rates[len(rates) // 2], 1), "max": round(rates[-1], 1),
               "launch_thread_s": {k: round(v, 3) for k, v in t.items()},
               "what": "wav (PCM16, tmpfs) -> decode -> pinned H2D -> forward (all layers: --use_n_layer --n_layer -1) -> last "
                       "state -> D2H -> .pt (tmpfs), one process, driver of preprocessing/preprocess_speech.py; weights already "
                       f"resident; median of {passes} timed passes after one that sizes the arenas and records the command lists"}
        if ref_rule:
            rec["reference_default_layer_rule"] = ref_rule
        return rec
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=8, help="batches replayed back to back per counted step")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--max_len", type=int, default=80, help="tokens per text (roberta workloads)")
    ap.add_argument("--ssl_type", type=str, default="microsoft/wavlm-large")
    ap.add_argument("--mode", type=str, default="bf16", choices=["bf16", "fp32x", "f16", "f16q", "f16a", "f16x", "f16m", "f16mf"])
    ap.add_argument("--parity-mode", type=str, default="f16mf,f16x,f16m,f16a,f16,fp32x",
                    help="numerics mode(s) of the parity records, comma separated: the first fills `parity_mode`, "
                         "the others `parity_mode_<name>`")
    ap.add_argument("--layers", type=int, default=0, help="debug: truncate the encoder (invalidates the metric)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the checks and the other measurements: output verification, roofline / "
                         "attention-block / step-decomposition legs, parity modes, end-to-end legs, other encoders, CPU baseline "
                         "(the --no-* options below drop single legs of a --full run; a plain run has none of them)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-trace", action="store_true", help="skip per-launch GEMM events")
    ap.add_argument("--no-verify", action="store_true", help="skip the output checks of the timed path")
    ap.add_argument("--no-parity", action="store_true", help="skip the parity_mode record (second encoder + oracle)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end (files on tmpfs) leg")
    ap.add_argument("--e2e-files", type=int, default=4096)
    ap.add_argument("--e2e-default-files", type=int, default=1024,
                    help="files of the second end-to-end leg, run in the drivers' DEFAULT numerics mode (0: skip)")
    ap.add_argument("--other-encoders", type=str, default="xlsr,hubert,whisper",
                    help="after the headline of a --full run: short verified runs (3 steps) of BASELINE configs[2..4]'s encoders on their own batch "
                         "shapes, in the timed mode AND in the tolerance-grade modes (f16mf, f16x, f16m: throughput + error against the CPU oracle), "
                         "comma separated from xlsr,hubert,whisper ('' or none: skip -- what every script under tools/ passes; xlsr adds "
                         "~1 min of weight generation)")
    ap.add_argument("--e2e-workers", type=int, default=4, help="host threads of the end-to-end leg (reference default 4)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--split", type=str, default="", help="explicit utterance-group sizes, e.g. 9,7 (overrides --micro)")
    ap.add_argument("--micro", type=int, default=0,
                    help="split every batch into this many utterance groups run as parallel graph branches")
    ap.add_argument("--inflight", type=int, default=0,
                    help="whole batches in flight at once, one hipGraph branch (HIP stream) each -- the drivers' two-slot pipeline; "
                         "--inflight 1 --micro 2 is the round-1/2 form (one batch split into two groups of 8)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps, write the hidden states the last timed step computed to DIR/*.npy "
                         "(rank 0; a fixed, seeded sample of the rows, < 64 MB: see dump_outputs)")
    args = ap.parse_args()
    if not args.full:                  # the headline alone: every leg after the timed region is off
        args.no_cpu_baseline = args.no_trace = args.no_verify = args.no_parity = args.no_e2e = True
        args.other_encoders = "none"

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
    # one process per GPU.  (local_rank % device_count is the identity on a full node; with SER_DIST_BACKEND=gloo it lets the
    # multi-rank control flow be rehearsed by N processes on ONE GPU, where RCCL would refuse two ranks on a device.)
    dev_index = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    import torch.distributed as dist
    from interspeech_ser_amd import dist as D
    D.init((os.environ.get("SER_DIST_BACKEND") or "nccl") if world > 1 else None, device)

    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import build_encoder
    geo = C.geometry_for(args.ssl_type)
    if args.layers:
        geo = C.with_layers(geo, args.layers)
    whisper = geo.family == C.FAMILY_WHISPER
    if geo.family in (C.FAMILY_ROBERTA, C.FAMILY_DEBERTA):
        return bench_text(args, geo, rank, world, device, D)
    num_samples = int(round(args.seconds * 16000))
    # defaults (0): two whole batches in flight for the wav2vec2-style encoders (WavLM-large +2.6..4.3 %, HuBERT-xlarge +2.6 %, XLS-R-2B
    # +5.6 % over one batch split in two groups, same box); Whisper's 30 s windows (M = 24 000 rows per batch) prefer one batch as two
    # groups of 8 (394 against 381 utt/s)
    if args.inflight <= 0:
        args.inflight = 1 if whisper else 2
    if args.micro <= 0:
        args.micro = 2 if (whisper and args.inflight == 1) else 1
    inflight = max(1, args.inflight)
    reps = max(1, args.reps // inflight)               # replays per counted step: a step stays `--reps` batches (8) back to back

    sd, bcast_s, bcast_bytes = broadcast_weights(geo, 0, rank)
    enc = build_encoder(geo, sd, device, args.mode)
    if world > 1:
        sd = None                  # views of the fp32 broadcast bucket: dropping them frees it (weights stay 1x in HBM)
        torch.cuda.empty_cache()
    batches_waves = [synth_batch(args.batch, num_samples, 1234 + rank + 7919 * j) for j in range(inflight)]
    waves = batches_waves[0]
    lengths = [num_samples] * args.batch

    # `inflight` whole batches run at once, each on its own branch of one hipGraph (round 3: measured +4.3 % over one batch
    # split into two groups of 8, same box -- the launches have the shape BASELINE.json's config names, batch = 16, and the
    # second batch fills what the first leaves idle).  `micro` > 1 additionally splits every batch into utterance groups.
    micro = args.micro if 1 < args.micro <= args.batch else 1
    per = -(-args.batch // micro)                                   # uneven splits allowed: 16 -> 6 + 5 + 5
    cuts = [round(i * args.batch / micro) for i in range(micro + 1)]
    if args.split:                                                  # explicit group sizes, e.g. --split 9,7
        sizes = [int(x) for x in args.split.split(",")]
        assert sum(sizes) == args.batch and min(sizes) > 0, "--split must add up to --batch"
        micro, cuts = len(sizes), [sum(sizes[:i]) for i in range(len(sizes) + 1)]
        per = max(sizes)
    spans = list(zip(cuts[:-1], cuts[1:]))
    branches = [(j, a, b) for j in range(inflight) for (a, b) in spans]       # one graph branch (slot, stream) each

    def make_groups(e):
        return [(e.upload(batches_waves[j][a:b], slot=slot), lengths[a:b]) for slot, (j, a, b) in enumerate(branches)]

    groups = make_groups(enc)
    torch.cuda.synchronize()

    def eager_step(e=enc, grp=groups):
        return [e.forward(w, l, slot=slot) for slot, (w, l) in enumerate(grp)]

    def timed(e, grp):
        """(elapsed seconds of `steps` counted steps, the HiddenStates the replayed graph writes into)"""
        if args.no_graph:
            hs_ref = [None]

            def one():
                hs_ref[0] = eager_step(e, grp)
            hs = None
        else:
            graph, hs = e.capture_concurrent(grp)
            one = graph.replay
        for _ in range(args.warmup):
            for _ in range(reps):
                one()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            for _ in range(reps):
                one()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        return dt, (hs if hs is not None else hs_ref[0])

    elapsed, hs_timed = timed(enc, groups)
    if rank == 0 and args.dump_outputs:                           # before any later leg re-uses the arenas
        dump_outputs(args.dump_outputs, hs_timed)

    # ---- verification of what was just timed (rank 0): the states the LAST replay left in HBM
    verification = None
    if rank == 0 and not args.no_verify:
        kept = [h.states.clone() for h in hs_timed]
        eager = eager_step()                                      # same arenas, command-list path, default stream
        torch.cuda.synchronize()
        same = all(torch.equal(k, e.states) for k, e in zip(kept, eager)) and \
            all(k_h.frame_offs == e.frame_offs for k_h, e in zip(hs_timed, eager))
        finite = all(bool(torch.isfinite(k).all()) for k in kept)
        verification = {"graph_replay_equals_eager_bitwise": bool(same), "all_finite": finite,
                        "states_checked": int(sum(k.shape[0] for k in kept)), "utterances": args.batch * inflight}
        from interspeech_ser_amd.engine import HiddenStates
        hs_timed = [HiddenStates(k, h.frame_offs) for k, h in zip(kept, hs_timed)]    # the timed graph's own results, kept
        del eager

    # Roofline leg: the same K steps again, launched eagerly with a HIP event pair around every
    # ser_gemm launch on the launch stream (events cannot be timed inside a replayed graph).
    trace = None
    if not args.no_trace:
        enc.gemm_trace = []
        for _ in range(args.steps):
            eager_step()
        torch.cuda.synchronize()
        trace, enc.gemm_trace = enc.gemm_trace, None
    # Attention-block leg (north_star target: >= 30 % of the bf16 MFMA peak on packed QKV projection -> attention ->
    # output projection): one more eager pass with one event pair per layer around exactly that sub-graph.
    blocks = blocks_full = blocks_conc = None
    if not args.no_trace and not whisper and geo.family != C.FAMILY_ROBERTA:
        enc.block_trace = []
        for _ in range(args.steps):
            eager_step()
        torch.cuda.synchronize()
        blocks, enc.block_trace = enc.block_trace, None
        # ... and once more with the whole batch in ONE launch per kernel (the shape BASELINE.json's config names)
        if micro > 1:
            packed = enc.upload(waves)
            enc.block_trace = []
            for _ in range(max(2, args.steps // 4)):
                enc.forward(packed, lengths, slot=len(groups))
            torch.cuda.synchronize()
            blocks_full, enc.block_trace = enc.block_trace, None
        # ... and the sub-graph alone the way the step runs it: both utterance groups' attention blocks at once, on two streams
        blocks_conc = None
        if len(groups) == 2 and not args.no_graph:
            # captured the way the step is: one hipGraph, one branch per group, replayed
            warm = torch.cuda.Stream(device=device)
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                for slot, (w, l) in enumerate(groups):
                    enc.attention_blocks_only(l, slot)
            torch.cuda.current_stream().wait_stream(warm)
            torch.cuda.synchronize()
            side = torch.cuda.Stream(device=device)
            gblk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gblk):
                main = torch.cuda.current_stream()
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    enc.attention_blocks_only(groups[1][1], 1)
                n_calls = enc.attention_blocks_only(groups[0][1], 0)
                main.wait_stream(side)
            gblk.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                gblk.replay()
            e1.record()
            torch.cuda.synchronize()
            blocks_conc = (e0.elapsed_time(e1) * 1e3 / 10 / n_calls, len(groups[0][1]) + len(groups[1][1]))

    # Step decomposition in the regime that is timed: the recorded command lists of the two utterance groups, filtered to ONE
    # class of kernels (GEMMs / attention / everything else), captured as the same two-branch hipGraph and replayed.  The per-class
    # times are what each class costs UNDER the step's concurrency (the eager roofline leg above times one launch at a time);
    # their sum is compared with the measured step.
    decomp = None
    if rank == 0 and not args.no_trace and not args.no_graph and len(groups) >= 1:
        from interspeech_ser_amd import _lib as L_
        classes = {"gemm": lambda op: op == L_.OP_GEMM, "attention": lambda op: op == L_.OP_ATTENTION,
                   "other": lambda op: op not in (L_.OP_GEMM, L_.OP_ATTENTION)}
        eager_step()                                                  # the tapes carry this batch's sizes
        torch.cuda.synchronize()
        decomp = {}
        for cname, keep in classes.items():
            subs = [enc.recorded_tape(l, slot).subset(keep) for slot, (w, l) in enumerate(groups)]
            sides_d = [torch.cuda.Stream(device=device) for _ in subs[1:]]
            for t in subs:                                            # warm-up outside the capture
                t.run({}, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            gd = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gd):
                main_s = torch.cuda.current_stream()
                for st in sides_d:
                    st.wait_stream(main_s)
                for t, st in zip(subs[1:], sides_d):
                    with torch.cuda.stream(st):
                        t.run({}, st.cuda_stream)
                subs[0].run({}, main_s.cuda_stream)
                for st in sides_d:
                    main_s.wait_stream(st)
            gd.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                gd.replay()
            e1.record()
            torch.cuda.synchronize()
            decomp[cname] = {"ms_per_batch": round(e0.elapsed_time(e1) / 10, 4), "launches_per_batch": int(sum(t.n for t in subs))}
            del gd

    elapsed = D.max_over_ranks(elapsed)
    e2e = e2e_default = None
    if not args.no_e2e:                                           # every rank: its own files, aggregated inside (weak scaling)
        e2e = end_to_end_leg(args, enc, geo, whisper, args.e2e_files, num_samples, world, D)

    if rank == 0:
        total_utts = args.batch * inflight * reps * args.steps * world
        value = total_utts / elapsed
        gf_utt = whisper_gflop_per_utt(geo) if whisper else algorithmic_gflop_per_utt(geo, num_samples)
        dtype_name = {"bf16": "bf16", "fp32x": "bf16x3 (bf16 hi + lo planes, 3 products)", "f16": "f16 (f16x3 stem)",
                      "f16q": "f16 (f16x3 stem and logit path)", "f16a": "f16 (f16x3 stem and attention block)",
                      "f16x": "f16x3 (fp16 hi + lo planes, 3 products)",
                      "f16m": "f16 + block-scaled e4m3 cross terms (2 product-equivalents; f16x3 stem, attention, output projection)",
                      "f16mf": "f16x3; FC1 / FC2 and, from a third of the depth on, the packed projection as f16 + block-scaled e4m3 cross terms"}
        out = {
            "metric": "utterances/sec (10 s @16 kHz) WavLM-large embed extract" if geo is C.WAVLM_LARGE and abs(args.seconds - 10) < 1e-6
                      else f"utterances/sec ({args.seconds:.0f} s @16 kHz) {geo.name} embed extract",
            "value": round(value, 2), "unit": "utterances/s",
            # the tolerance-grade figures next to the headline (filled below from `parity_mode`: the drivers' default numerics, and the
            # fastest mode inside north_star's 1e-3), so that a truncated line still shows them
            "parity_value": None, "parity_mode_name": None, "parity_err": None,
            "fast_parity_value": None, "fast_parity_mode_name": None, "fast_parity_err": None,
            "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype_name[args.mode], "data": "synthetic",
            "config": {"workload": f"{geo.name} embed extract, batch={args.batch} x {args.seconds:.0f} s @16 kHz per GPU, "
                                   f"all {geo.num_layers + 1} hidden states to HBM, mode={args.mode}; a counted step = "
                                   f"{reps * inflight} such batches ({args.batch * reps * inflight} utterances per GPU), "
                                   f"{inflight} in flight at a time",
                       "batch": args.batch, "batches_per_step": reps * inflight, "batches_in_flight": inflight,
                       "ms_per_batch": round(1e3 * elapsed / args.steps / reps / inflight, 3),
                       "frames_per_utt": geo.max_source_positions if whisper else geo.frames_for(num_samples), "gflop_per_utt": round(gf_utt, 1),
                       "parallelism": f"utterance-sharded x{world}, " + ("no collective (one process)" if world == 1 else
                                      f"one weight broadcast over {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()} only")},
            "achieved_tflops_whole_path": round(value * gf_utt / 1e3 / world, 1),
            "launch": "eager" if args.no_graph else f"hipGraph replay, {len(branches)} concurrent branch(es): {inflight} batch(es) in flight x "
                                                    f"{micro} utterance group(s) of {per}",
            "weight_broadcast_s": round(bcast_s, 4),
            "collective": collective_record(world, bcast_s, bcast_bytes),
        }
        if trace:
            dur_ms = sum(t[0].elapsed_time(t[1]) for t in trace)
            flops = sum(t[2] for t in trace)
            algo_bytes = sum(t[3] for t in trace)
            # HBM bytes per launch: only from a PMC summary taken with THESE kernel sources on THIS workload
            traffic, traffic_note = None, "no rocprofv3 PMC summary for these kernel sources / this workload under profiles/"
            key = f"{geo.name}|{args.mode}|batch={args.batch}x{args.seconds:.0f}s|inflight={inflight}|groups={micro}"
            for fn in sorted(os.listdir(os.path.join(ROOT, "profiles")), reverse=True):
                if fn.endswith("pmc_traffic.json"):
                    rec = json.load(open(os.path.join(ROOT, "profiles", fn)))
                    if rec.get("kernel_source_digest") == kernel_source_digest() and rec.get("workload_key") == key:
                        traffic = rec["hbm_bytes_per_launch"]
                        traffic_note = (f"HBM bytes per ser_gemm launch from separate rocprofv3 PMC passes (FETCH_SIZE x2 + WRITE_SIZE, "
                                        f"profiles/{fn}), same command run eagerly, same kernel sources ({rec['kernel_source_digest']})")
                        break
            n = len(trace)
            achieved = flops / (dur_ms * 1e-3) / 1e12
            mult = sum(t[2] * t[4] for t in trace) / max(flops, 1.0)      # MFMA products per algorithmic FLOP, per launch from its mode (3 on two planes)
            out["roofline"] = {
                "kernel": "ser_gemm_kernel (bf16 MFMA implicit-conv GEMM + fused epilogue)",
                "bound": "mfma", "achieved": round(achieved, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                "regime": "one launch at a time (replaced below by the step's own regime when the decomposition leg ran)",
                "traffic_note": traffic_note,
                "algorithmic_bytes_per_launch": round(algo_bytes / n),
                "launches": n, "avg_launch_us": round(1e3 * dur_ms / n, 2),
                "algorithmic_gflop_per_launch": round(flops / n / 1e9, 2),
                "mfma_products_per_algorithmic_flop": round(mult, 3),
                "gemm_ms_per_batch": round(dur_ms / args.steps / inflight, 3),
                "under_step_concurrency": None,
                "measured": "HIP events around every ser_gemm launch, eager pass of K batches right after the timed region "
                            "(one launch at a time: no concurrent utterance group)",
                "clock_note": "peak is the nominal 2.4 GHz figure; a diagnostic build (tools/gemm_clock.py, profiles/r02_gemm_inkernel_clock.txt) "
                              "stamps 1.92-1.97 GHz held inside the 256x256 K loop on random operands, where it runs at 69-73 % of the matrix "
                              "pipe at that clock; not measured in this run",
                "board_note": "not measured in this run: tools/energy_probe.hip (profiles/r05_energy_probe.txt) -- the matrix pipe alone, register "
                              "operands, all 256 CUs, sustains 2 220-2 290 TFLOP/s at 1 340-1 370 W of this board's 1 400 W (sclk ~2.2 GHz), a loop of "
                              "the 256x256 tile's shape with LDS fragment reads and L2 -> LDS fills 1 596; `peak` stays the nominal figure",
            }
        if decomp:
            ms_batch = 1e3 * elapsed / args.steps / reps / inflight
            for v in decomp.values():                                  # a replay covers `inflight` batches
                v["ms_per_batch"] = round(v["ms_per_batch"] / inflight, 4)
                v["launches_per_batch"] //= inflight
            total = sum(v["ms_per_batch"] for v in decomp.values())
            out["step_decomposition"] = {
                "classes": decomp, "sum_ms_per_batch": round(total, 4), "measured_ms_per_batch": round(ms_batch, 4),
                "sum_over_measured": round(total / ms_batch, 4),
                "measured": "each class = the step's own recorded command lists filtered to that class of kernels, captured as the same "
                            "two-branch hipGraph (one branch per utterance group) and replayed 10x between HIP events; a class runs without "
                            "the other classes between its launches, so the sum can differ from the step by what cross-class overlap or "
                            "dependency bubbles are worth"}
            if trace and "roofline" in out:
                gflop_batch = sum(t[2] for t in trace) / args.steps / inflight / 1e9
                ach_c = gflop_batch / decomp["gemm"]["ms_per_batch"]          # GF per ms = TF/s
                r = out["roofline"]
                # `achieved` / `frac` = the regime `value` is measured in (the GEMM launches of a batch as the step's concurrent graph
                # branches run them); the one-launch-at-a-time figure the per-launch events give stays beside it: sum of those launch
                # durations EXCEEDS the batch time, so it cannot be the step's figure (round-3 verdict, weak #6)
                r["one_launch_at_a_time"] = {"achieved": r["achieved"], "frac": r["frac"], "avg_launch_us": r["avg_launch_us"],
                                             "gemm_ms_per_batch": r["gemm_ms_per_batch"], "measured": r["measured"],
                                             "rocprof": "profiles/r05_kernel_trace_one_launch_at_a_time_wavlm_large_bf16.csv (same command with "
                                                        "--no-graph --inflight 1 --micro 1)"}
                r["achieved"], r["frac"] = round(ach_c, 1), round(ach_c / MFMA_BF16_PEAK_TFLOPS, 4)
                r["gemm_ms_per_batch"] = decomp["gemm"]["ms_per_batch"]
                r["avg_launch_us"] = round(1e3 * decomp["gemm"]["ms_per_batch"] / max(decomp["gemm"]["launches_per_batch"], 1), 2)
                r["regime"] = "the step's own: the ser_gemm launches of a batch on the concurrent branches of one hipGraph, as timed for `value`"
                r["measured"] = ("algorithmic FLOPs of a batch's ser_gemm launches / replay time per batch of the GEMM-only command lists "
                                 "captured as the step's concurrent graph branches (HIP events around 10 replays); avg_launch_us = that time / launches")
                r["under_step_concurrency"] = {"achieved": r["achieved"], "frac": r["frac"], "unit": "TFLOP/s",
                                               "gemm_ms_per_batch": r["gemm_ms_per_batch"]}
        if blocks:
            T = geo.frames_for(num_samples)
            Dm, dh = geo.hidden, geo.head_dim
            gf_block = (2.0 * T * Dm * 3 * Dm + 2.0 * T * Dm * Dm + 4.0 * T * T * Dm) / 1e9       # q,k,v + out + QK^T + PV, per utterance
            us = sum(b[0].elapsed_time(b[1]) for b in blocks) * 1e3 / len(blocks)
            utts = blocks[0][2]
            ach = gf_block * utts / us * 1e3                       # GF per us -> TF/s
            out["attention_block"] = {
                "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4),
                "target_frac": 0.30, "us_per_layer_call": round(us, 2), "utterances_per_launch": utts,
                "algorithmic_gflop_per_utt_layer": round(gf_block, 3), "layer_calls": len(blocks),
                "measured": "HIP events around QKV GEMM -> ser_attention -> out-proj GEMM of every layer, eager pass, "
                            "one utterance group at a time (no concurrent group)",
            }
            if blocks_full:
                us_f = sum(b[0].elapsed_time(b[1]) for b in blocks_full) * 1e3 / len(blocks_full)
                ach_f = gf_block * blocks_full[0][2] / us_f * 1e3
                out["attention_block"]["whole_batch_per_launch"] = {
                    "utterances_per_launch": blocks_full[0][2], "us_per_layer_call": round(us_f, 2),
                    "achieved": round(ach_f, 1), "frac": round(ach_f / MFMA_BF16_PEAK_TFLOPS, 4)}
            if blocks_conc:
                us_c, utts_c = blocks_conc
                ach_c = gf_block * utts_c / us_c * 1e3
                out["attention_block"]["two_concurrent_groups"] = {
                    "utterances_per_layer_call": utts_c, "us_per_layer_call": round(us_c, 2), "achieved": round(ach_c, 1),
                    "frac": round(ach_c / MFMA_BF16_PEAK_TFLOPS, 4),
                    "measured": "the sub-graph alone (no FFN between the blocks) captured like the timed step: one hipGraph with one "
                                "branch per concurrent group / batch, HIP events around 10 replays of all layers"}

        # ---- parity_mode: throughput + measured errors of the mode that meets north_star's 1e-3 (rank 0, N = 1)
        checks_ok = verification is not None and verification["graph_replay_equals_eager_bitwise"] and verification["all_finite"]
        if world == 1 and not args.no_parity and verification is not None:
            first = [f"batch {j} utterance {a}" for j, a, _ in branches]     # first utterance of every branch
            ref = oracle_states(geo, sd, waves[0], whisper)               # CPU oracle on utterance 0 (full geometry, T frames)
            err_m = max(rel_err(hs_timed[0].utterance(0, l).cpu(), r) for l, r in enumerate(ref))
            bound = {"bf16": 3e-2, "fp32x": 1e-3, "f16": 1e-3, "f16q": 1e-3, "f16a": 1e-3, "f16x": 1e-3, "f16m": 1e-3, "f16mf": 1e-3}[args.mode]
            verification.update({"weights": "seeded synthetic weights of the named geometry (no checkpoint can be fetched offline): every error "
                                            "below is on those; stress fixtures (LoRA-scaled queries, sharp attention, outlier channels) are in tests/",
                                 "timed_mode": args.mode, "timed_mode_max_rel_err_vs_oracle": float(f"{err_m:.3e}"),
                                 "timed_mode_bound": bound, "utterances_vs_parity_mode": first})
            checks_ok = checks_ok and err_m <= bound
            what = {"fp32x": "bf16 x3 split (hi*hi + lo*hi + hi*lo) everywhere",
                    "f16x": "the same 3-product split everywhere on fp16 hi + lo planes (22-bit operands instead of 16; the drivers' default of "
                            "round 4: <= 1.0e-4 on the full-depth stress cases of profiles/r04_depth_envelope.txt)",
                    "f16m": "round 5: packed projection, FC1 and FC2 as fp16 main product + block-scaled e4m3 cross terms on "
                            "v_mfma_scale_f32_16x16x128_f8f6f4 (x_hi w_hi + x_lo w_8 + x_8 w_lo: 2 product-equivalents instead of 3, operand error "
                            "~2^-15); conv stem, attention and output projection on the fp16 hi + lo split (full-depth stress cases: "
                            "profiles/r05_depth_envelope_f16m*.txt, <= 4.8e-4, inside fp32x's on every case)",
                    "f16mf": "round 5, the drivers' default: f16x with the feed-forward pair (FC1, FC2: 2/3 of the layer FLOPs) of every layer and "
                             "the packed projection from a third of the depth on in f16m's operand format; conv stem, attention, output "
                             "projection and the first third's packed projections on the fp16 hi + lo split (full-depth stress "
                             "cases, all four encoder families: profiles/r05_depth_envelope_f16mf.txt, <= 2.2e-4, 2-7x inside fp32x's on every case)",
                    "f16": "fp32x conv stem (conv stack, projection, positional conv) + fp16 single-product encoder layers",
                    "f16a": "fp32x conv stem; packed QKV projection, attention (S = K Q^T, P V) and output projection on the 3-product "
                            "split over fp16 hi + lo planes; FC1 / FC2 (62 % of the layer FLOPs) single-product fp16",
                    "f16q": "f16 with the logit path fp32-grade: q / k (+ gate) columns of the packed projection and S = K Q^T on the "
                            "3-product split over fp16 hi + lo planes; v, P V, output projection and feed-forward single-product fp16",
                    "bf16": "bf16 single product everywhere"}
            for idx, pmode in enumerate(m for m in args.parity_mode.split(",") if m):
                if pmode == args.mode:
                    enc_p, hs_p, el_p = enc, hs_timed, elapsed
                else:
                    enc_p = build_encoder(geo, sd, device, pmode)
                    grp_p = make_groups(enc_p)
                    torch.cuda.synchronize()
                    el_p, hs_p = timed(enc_p, grp_p)
                err_mode = max(states_err(hs_timed[g], 0, hs_p[g], 0) for g in range(len(branches)))
                err_p = max(rel_err(hs_p[0].utterance(0, l).cpu(), r) for l, r in enumerate(ref))
                out["parity_mode" if idx == 0 else f"parity_mode_{pmode}"] = {
                    "mode": pmode, "arithmetic": what[pmode],
                    "value": round(args.batch * inflight * reps * args.steps / el_p, 2), "unit": "utterances/s",
                    "ms_per_batch": round(1e3 * el_p / args.steps / reps / inflight, 3),
                    "max_rel_err_vs_oracle": float(f"{err_p:.3e}"), "tolerance": 1e-3, "within_tolerance": bool(err_p <= 1e-3),
                    "timed_mode_max_rel_err_vs_this_mode": float(f"{err_mode:.3e}"),
                    "oracle_sample": f"utterance 0 ({args.seconds:.0f} s, all {geo.num_layers + 1} states, {ref[0].shape[0]} frames), fp32 PyTorch-CPU oracle",
                    "error_form": "max|a-b| / max(1, max|b|) per hidden state, worst state",
                }
                checks_ok = checks_ok and err_p <= 1e-3 and err_mode <= max(bound, 1e-3)
                if pmode == DRIVER_DEFAULT_MODE and not args.no_e2e and args.e2e_default_files > 0:
                    # the file-to-file leg in the numerics the drivers default to (preprocessing/preprocess_speech.py without --mode)
                    e2e_default = end_to_end_leg(args, enc_p, geo, whisper, args.e2e_default_files, num_samples, 1, D,
                                                 mode=pmode, passes=2, with_ref_rule=False)
                if enc_p is not enc:
                    del enc_p, hs_p
                    torch.cuda.empty_cache()
            precs = [v for k, v in out.items() if k.startswith("parity_mode") and isinstance(v, dict)]
            verification["parity_modes_within_1e-3_of_oracle"] = bool(all(v["within_tolerance"] for v in precs))
            if precs:
                first = out["parity_mode"]
                out["parity_value"], out["parity_mode_name"], out["parity_err"] = first["value"], first["mode"], first["max_rel_err_vs_oracle"]
                # ... among the modes that hold the 1e-3 gate at FULL DEPTH under the stress weights too (tests/test_gpu_depth.py): on the
                # bench's Gaussian weights f16 / f16a are inside 1e-3 as well, under sharp attention at 24 layers they are not
                ok = [v for v in precs if v["within_tolerance"] and v["mode"] in ("f16mf", "f16x", "f16m", "fp32x")]
                if ok:
                    best = max(ok, key=lambda v: v["value"])
                    out["fast_parity_value"], out["fast_parity_mode_name"], out["fast_parity_err"] = best["value"], best["mode"], best["max_rel_err_vs_oracle"]
        if verification is not None:
            out["verified"] = bool(checks_ok)
            out["verification"] = verification
        if e2e is not None:
            out["end_to_end"] = e2e
        if e2e_default is not None:
            out["end_to_end_default_mode"] = e2e_default
        if world == 1 and args.other_encoders and args.other_encoders != "none":
            del enc, hs_timed, groups
            torch.cuda.empty_cache()
            out["other_encoders"] = {n: other_encoder_run(n, device, args.mode) for n in args.other_encoders.split(",") if n in OTHER_ENCODERS}
            if "verified" in out:                     # a failed check of any encoder fails the line
                out["verified"] = bool(out["verified"] and all(v["verified"] for v in out["other_encoders"].values()))
        if world == 1 and not args.no_cpu_baseline and not whisper:
            out["cpu_baseline"] = cpu_baseline(geo, sd, num_samples)
        print(json.dumps(out), flush=True)
    D.shutdown()


if __name__ == "__main__":
    main()
