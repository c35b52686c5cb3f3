"""Extraction drivers: the counterparts of the reference's two scripts.

``run_speech`` mirrors preprocessing/preprocess_speech.py and ``run_whisper``
mirrors preprocessing/preprocess_whisper.py: same flags (:13-22 / :14-23), same
stdout lines, same ``<save_path>/<basename>.pt`` files holding a bare [T, D]
float32 CPU tensor, exit status 0 with per-file failures printed and skipped
(:45-73).  What changes is underneath: files are length-bucketed into ragged
batches, each batch is one packed forward on the GPU through libserhip, decode
and ``torch.save`` run in ``--num_workers`` host threads around it, and with
``torchrun`` the file list is sharded over ranks (one process per GPU).

Layer selection is the reference's (a19):
* speech script: ``--n_layer`` is parsed and NOT used; the state written is ``hidden_states[N]`` with N = the number of
  files found in ``--save_path`` at start-up (preprocess_speech.py:41,67) -- hidden_states[0] for the README's recipe on a
  fresh directory (README.md:71).  That rule is the default here too (N is taken once, on rank 0, before any rank writes);
  the additive flag ``--use_n_layer`` switches to ``hidden_states[--n_layer]``.  One stdout line says which rule is active.
* whisper script: ``hidden_states[--n_layer]`` (preprocess_whisper.py:71), default -1.
Either way the forward stops after the state it needs (``last_state``): layers that only feed later states are not launched.
Additive flags: ``--batch_size``, ``--mode``, ``--checkpoint``, ``--synthetic_weights``, ``--skip_existing``,
``--use_n_layer``, ``--save_format``, ``--resample``, ``--lora_alpha``, ``--timing``.  ``--seed`` (parsed and unused by the
reference) seeds the synthetic weights.
"""
from __future__ import annotations

import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import SlotPipeline, make_batches, prefetch       # noqa: F401  (make_batches: tests and tools import it from here)
from .frontend import (RESAMPLE_MAX_R, TARGET_SR, decode_wav, feature_path, host_resample, load_wav_16k, resample_ratio,
                       resampled_len, save_feature, whisper_saved_rows)


# ------------------------------------------------------------------------------- CLI
def build_parser(whisper: bool) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    # the reference's flags, names and defaults unchanged (preprocess_speech.py:13-22)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--ssl_type", type=str, default="wavlm-large")
    p.add_argument("--save_path", type=str, default="./")
    p.add_argument("--wav_dir", type=str, default="./")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--n_layer", type=int, default=-1)
    p.add_argument("--use_average", type=str, default="n")
    # additive
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--mode", type=str, default="f16mf", choices=["f16mf", "f16x", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16"],
                   help="numerics of the matrix products (errors: max|a-b| / max(1, max|b|) per hidden state against the fp32 reference, all "
                        "states, FULL depth, profiles/r04_depth_envelope*.txt, r05_depth_envelope_f16m*.txt).  f16mf (default since round 5): the "
                        "3-product split on fp16 hi + lo planes for the conv stem, attention, output projection and the first third's packed projections; "
                        "FC1 / FC2 (2/3 of the layer FLOPs) and the later layers' packed projections as fp16 main product + block-scaled e4m3 cross "
                        "terms on the gfx950 scaled matrix instruction -- 1.5e-5 "
                        "on Gaussian weights, <= 2.2e-4 under sharp attention / LoRA-scaled queries / outlier channels at 24, 32 and 48 layers in "
                        "all four encoder families (2-7x inside fp32x's on every case), 1.15x f16x's throughput.  f16x (the default of round 4): "
                        "the 3-product split everywhere -- 4e-6 plain, <= 1.5e-4 under the stress cases: the widest margin.  All fp16-plane modes: "
                        "operand values must stay below 65 504 (every kernel that rounds to such a plane reports into a guard "
                        "word read back with every batch, and a batch that saturates FAILS its files).  f16m (round 5): packed projection / FC1 / FC2 "
                        "as fp16 main product + block-scaled e4m3 cross terms on the gfx950 scaled matrix instruction -- 1.1x faster than f16x, 2e-5 "
                        "plain, <= 4.8e-4 under the stress cases (inside fp32x's on every one), fp16 range.  fp32x: the same split as f16x on bf16 "
                        "planes -- fp32 range, 2e-5 plain, <= 8e-4 under the stress cases.  f16a: fp16 single products in the feed-forward, 1.35x faster, 4e-4 plain "
                        "but 3e-3 under sharp attention at depth (outside the 1e-3 gate: was the default in round 3).  f16q / f16: faster, "
                        "7e-4 plain, 1e-2 under stress.  bf16: fastest (~1e-2).  Limits: utterances of at least 400 samples (the conv stack's "
                        "receptive field); no upper limit (WavLM utterances beyond ~2 min read their relative-position bias from global memory)")
    p.add_argument("--checkpoint", type=str, default="",
                   help="local *.safetensors / pytorch_model.bin (or directory); default: HF cache lookup, "
                        "else seeded synthetic weights")
    p.add_argument("--skip_existing", action="store_true")
    p.add_argument("--save_format", type=str, default="pt", choices=["pt", "npy"],
                   help="pt (default): what the reference writes and its heads read (torch.save of a [T, D] float32 tensor); "
                        "npy: the same array as <name>.npy for consumers without torch")
    p.add_argument("--resample", action="store_true",
                   help="accept non-16 kHz wav files through a Kaiser polyphase resampler that runs on the GPU ahead of the forward "
                        "(parity with librosa's soxr_hq unpinned)")
    p.add_argument("--lora_alpha", type=float, default=16.0,
                   help="LoRA alpha of a fine-tuned --checkpoint (the reference's LoraConfig: r=8, alpha=16)")
    p.add_argument("--timing", action="store_true", help="print where the launching thread spent its time")
    p.add_argument("--use_n_layer", action="store_true",
                   help="speech driver: write hidden_states[--n_layer] instead of the reference's rule, hidden_states[number of "
                        "files found in --save_path at start-up] (preprocess_speech.py:41,67); the whisper driver always honours "
                        "--n_layer, like the reference's")
    p.add_argument("--compat_layer_quirk", action="store_true",
                   help="accepted for older command lines: the reference's layer rule is the default now")
    p.add_argument("--synthetic_weights", action="store_true",
                   help="use seeded random weights of the right geometry (no network / benchmarking)")
    return p


from .dist import shard_files          # noqa: E402  (re-exported: the sharding rule lives in dist.py)


def resolve_layer_index(n_layer: int, num_states: int) -> int:
    idx = n_layer if n_layer >= 0 else num_states + n_layer
    if not 0 <= idx < num_states:
        raise IndexError("tuple index out of range")     # what hidden_states[N] raises in the reference
    return idx


# ------------------------------------------------------------------------ weights
def find_weights(ssl_type: str, checkpoint: str, synthetic: bool, seed: int, geo, lora_alpha: float = 16.0, keep: tuple = ()):
    """Rank 0 only: the other ranks receive the tensors by broadcast (dist.broadcast_state_dict).
    A checkpoint that carries PEFT LoRA adapters (preprocess_speech_pretrained.py:108-177) is merged at load.
    ``keep``: name prefixes ``weights.normalize_names`` leaves in (the CTC drivers' ``lm_head.``)."""
    from .weights import load_checkpoint, synthetic_state_dict
    if checkpoint:
        return load_checkpoint(checkpoint, lora_alpha, keep), f"checkpoint {checkpoint}"
    if not synthetic and os.path.isdir(ssl_type):         # --ssl_type may be a local snapshot directory, as with from_pretrained
        return load_checkpoint(ssl_type, lora_alpha, keep), f"snapshot {ssl_type}"
    if not synthetic:
        # offline HF cache layout: $HF_HOME/hub/models--org--name/snapshots/<rev>/
        home = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
        snap = os.path.join(home, "hub", "models--" + ssl_type.replace("/", "--"), "snapshots")
        if os.path.isdir(snap):
            for rev in sorted(os.listdir(snap)):
                try:
                    return load_checkpoint(os.path.join(snap, rev), keep=keep), f"HF cache {rev}"
                except OSError:
                    continue
        raise OSError(f"no local checkpoint for {ssl_type} (pass --checkpoint or --synthetic_weights)")
    return synthetic_state_dict(geo, seed), f"synthetic weights (seed {seed})"


# ------------------------------------------------------------------------ the loop
class _Extractor:
    def __init__(self, args, whisper: bool, device: str):
        from .engine import build_encoder
        self.args, self.whisper = args, whisper
        self.geo = C.resolve_geometry(args.ssl_type, args.checkpoint)      # config.json of the checkpoint, else the built-in table
        self.geo = C.resolve_fbank(self.geo, args.ssl_type, args.checkpoint)   # w2v-BERT: mel count and stacking of preprocessor_config.json
        if whisper != (self.geo.family == C.FAMILY_WHISPER):
            raise OSError(f"{args.ssl_type} is not a {'whisper' if whisper else 'wav2vec2-style'} encoder")
        from . import dist as D
        rank = D.env()[0]
        sd, err = None, ""
        self.weight_source = "broadcast from rank 0"
        if rank == 0:
            try:
                sd, self.weight_source = find_weights(args.ssl_type, args.checkpoint, args.synthetic_weights,
                                                      args.seed, self.geo, args.lora_alpha)
            except OSError as e:
                err = str(e)
        if D.broadcast_int(1 if (rank == 0 and sd is None) else 0) == 1:
            raise OSError(err or "rank 0 found no checkpoint")
        sd, self.bcast_s, self.bcast_bytes = D.broadcast_state_dict(sd)
        args.mode = self.supported_mode(self.geo, args.mode, whisper, args.ssl_type)
        normalize = True if whisper else C.resolve_do_normalize(args.ssl_type, args.checkpoint)   # AutoFeatureExtractor's do_normalize
        self.enc = build_encoder(self.geo, sd, device, args.mode, normalize=normalize)
        del sd                                                # the fp32 broadcast bucket (views of it) is not needed any more
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        self.average = args.use_average == "y"

    @staticmethod
    def supported_mode(geo, mode: str, whisper: bool, name: str) -> str:
        """``mode``, or the mode that runs instead on this geometry (said in one printed line)."""
        from .engine import POST_LN_MODES
        if mode in ("f16mf", "f16m") and (geo.hidden % 64 or geo.ffn % 64):
            # the block-scaled cross-term format works on 64-deep K tiles: a geometry whose widths are not multiples of 64 (none of the
            # reference's four) runs the 3-product split everywhere instead -- same or better parity, ~10 % slower
            print(f"--mode {mode} needs hidden / feed-forward widths that are multiples of 64 (here {geo.hidden} / {geo.ffn}): using f16x")
            mode = "f16x"
        if not whisper and not geo.stable_layer_norm and mode not in POST_LN_MODES:
            # the post-LayerNorm (*-base) encoders run the text encoders' modes; the others need FP16M copies out of ser_layernorm
            print(f"--mode {mode} is not implemented for post-LayerNorm encoders ({name}): using f16x")
            mode = "f16x"
        if geo.family in (C.FAMILY_W2V_BERT, C.FAMILY_W2V_CONFORMER) and mode not in POST_LN_MODES:
            # the conformer layers run ser_layernorm between their GEMMs, like the post-LayerNorm encoders: the same three modes
            print(f"--mode {mode} is not implemented for the conformer encoder ({name}): using f16x")
            mode = "f16x"
        return mode

    @classmethod
    def from_encoder(cls, args, enc, whisper: bool, weight_source: str = "caller's encoder"):
        """Wrap an encoder the caller already built (bench.py's end-to-end leg, tests): no weight search, no broadcast."""
        ex = cls.__new__(cls)
        ex.args, ex.whisper, ex.geo, ex.enc = args, whisper, enc.geo, enc
        ex.weight_source, ex.bcast_s, ex.bcast_bytes = weight_source, 0.0, 0
        ex.average = args.use_average == "y"
        return ex

    def upload_resampled(self, waves: List[np.ndarray], rates: Optional[Sequence[int]], slot: int = 0):
        """(packed 16 kHz device buffer, lengths at 16 kHz) of one batch.  ``rates`` (``--resample``): the files' own sample rates, the
        raw samples go up and ser_resample_v brings them to 16 kHz on the current stream; None: 16 kHz samples, plain upload."""
        if rates is None:
            return self.enc.upload(waves, slot), [len(w) for w in waves]
        return self.enc.upload_resampled(waves, rates, slot)

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        """The device rows of a forward that go back to the host: one hidden state or the mean of the last four (a subclass may put
        further device work here, on the current stream; baseline.BaselinePredictor runs its head)."""
        from .engine import mean_last4
        return mean_last4(hs) if self.average else hs.states[layer_index]

    def extract(self, waves: List[np.ndarray], layer_index: int, rates: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """One ragged batch -> one CPU [T, D] tensor per utterance (rows a19/a20), synchronously."""
        dev, lengths = self.upload_resampled(waves, rates)
        hs = self.enc.forward(dev, lengths, last_state=None if self.average else layer_index)
        self._check_range(hs.take_range_bits())
        sel = self.select(hs, layer_index)
        out = []
        host = self.enc.download(sel)
        for b, n in enumerate(lengths):
            rows = host[hs.frame_offs[b]: hs.frame_offs[b + 1]]
            if self.whisper:
                rows = rows[: whisper_saved_rows(n, rows.shape[1])]
            out.append(rows)
        return out

    # ---- fp16 range guard.  The default mode "f16mf" (and f16x / f16m / f16a / f16q / f16) keeps its operand copies on fp16 planes, which saturate
    # at +-65 504; every validation so far is on synthetic weights (|residual stream| <= ~1e3 even with the 1000x outlier-channel stress), and
    # wav2vec2-style checkpoints are known for massive activations.  Round 5: EVERY kernel that rounds a value to such a plane -- GEMM
    # epilogues (the FC1 / GELU output, q / k / v, the operand copies of the residual stream), the LayerNorm / centring / framing row
    # kernels -- ORs into one device word per pipeline slot (bit 0: beyond the range, bit 1: beyond half of it) at the price of one max per
    # value; the word comes back with EVERY batch's features.  Beyond the range the batch's files fail like any other per-file error
    # ("Failed to process ...: ... use --mode fp32x") instead of being written clipped; beyond half of it the run warns once.
    # (Round 4 reduced max|hidden state| with a torch pass on the first four batches and every 32nd, and saw the layer outputs only.)
    F16_LIMIT = 65504.0

    def _check_range(self, bits) -> None:
        bits = int(bits or 0)
        if bits:
            self.__dict__["range_bits_seen"] = self.__dict__.get("range_bits_seen", 0) | bits
        if bits & 1:
            raise ValueError(f"a value beyond the fp16 operand range of --mode {self.enc.mode_name} ({self.F16_LIMIT:.0f}) was met inside the "
                             f"forward (it would have been saturated): re-run with --mode fp32x (bf16 planes, fp32 range)")
        if bits & 2 and not self.__dict__.get("_range_warned"):
            self.__dict__["_range_warned"] = True
            print(f"WARNING: values within a factor 2 of the fp16 operand range of --mode {self.enc.mode_name} ({self.F16_LIMIT:.0f}); "
                  f"--mode fp32x has fp32 range")

    # ---- pipelined form: SLOTS slots (arena + HIP stream each), so batch i+1 is uploaded and launched while batch i
    # still computes, and its D2H copy / slicing / torch.save overlap the next forward.  The kernels of at most RUNNING
    # batches share the GPU (the regime bench.py times: two whole batches in flight).  SER_PIPE_SLOTS=3 keeps a third batch
    # uploaded and enqueued behind an event, so the GPU never drops to ONE batch while the launching thread collects a
    # finished one; measured (tools/pipe_slots_ab.sh, two A/B pairs on one box): 1 866 / 1 866 -> 1 881 / 1 888 utt/s end to
    # end at full depth, but 5 617 / 5 239 -> 4 812 / 4 993 for the reference's default rule (stem only, host-bound) -- so
    # two slots stay the default.  What separates the end-to-end rate from the kernels' 2 015 is stream launches instead of
    # a replayed hipGraph (ragged batches change every launch's sizes), not an idle GPU: the launching thread waits.
    # (2 or 3: the per-slot plan caches and tickets are sized for that; more slots would evict live plans every batch)
    SLOTS = min(3, max(2, int(os.environ.get("SER_PIPE_SLOTS", "2"))))
    RUNNING = 2

    def submit(self, waves: List[np.ndarray], layer_index: int, slot: int, rates: Optional[Sequence[int]] = None):
        """Enqueue upload -> forward -> selection -> D2H of one ragged batch on slot ``slot``'s stream; returns a
        ticket for ``collect``.  Nothing here waits for the GPU."""
        st = self.__dict__.setdefault("_streams", {})
        if slot not in st:
            st[slot] = torch.cuda.Stream(device=self.enc.device)
        tm = self.__dict__.setdefault("tm", dict(upload=0.0, upload_resample=0.0, forward=0.0, d2h=0.0))
        clock = time.perf_counter
        computed = self.__dict__.setdefault("_computed", [])      # "kernels done" events of the batches submitted so far, oldest first
        with torch.cuda.stream(st[slot]):
            t0 = clock()
            dev, lengths = self.upload_resampled(waves, rates, slot)     # lengths: at 16 kHz
            t1 = clock()
            if len(computed) >= self.RUNNING:                     # start once the batch RUNNING places ahead has left the compute units
                st[slot].wait_event(computed[-self.RUNNING])
            hs = self.enc.forward(dev, lengths, slot=slot, last_state=None if self.average else layer_index)
            t2 = clock()
            sel = self.select(hs, layer_index, slot)
            watch = None
            if hs.range_flag is not None:                         # the slot's guard word, read back with the features and cleared
                watch = self.__dict__.setdefault("_range_pin", {}).get(slot)
                if watch is None:
                    watch = self.__dict__["_range_pin"][slot] = torch.zeros(1, dtype=torch.int32).pin_memory()
                hs.take_range_bits(watch)
            ce = torch.cuda.Event()
            ce.record()
            computed.append(ce)
            del computed[: -self.SLOTS]
            host = self._pinned_out(slot, sel.shape[0], sel.shape[1])
            host.copy_(sel, non_blocking=True)
            evt = torch.cuda.Event()
            evt.record()
            t3 = clock()
        # upload_resample: the batches that went through ser_resample_v (raw samples H2D, its O(B) tables, the launch)
        tm["upload" if rates is None or all(r == TARGET_SR for r in rates) else "upload_resample"] += t1 - t0
        tm["forward"] += t2 - t1
        tm["d2h"] += t3 - t2
        return dict(slot=slot, event=evt, host=host, frame_offs=list(hs.frame_offs), lengths=lengths, watch=watch)

    def collect(self, ticket) -> List[torch.Tensor]:
        """Wait for a ticket's D2H copy; one [T, D] view of the slot's pinned buffer per utterance (valid until
        the slot's next ``submit``; ``hold`` defers that until the given futures are done)."""
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))            # raises -> the driver retries the batch per utterance and logs each failure
        host, fo = ticket["host"], ticket["frame_offs"]
        rows = [host[fo[b]: fo[b + 1]] for b in range(len(ticket["lengths"]))]
        if self.whisper:                                      # a20: min(ceil(len / 320), D) rows (preprocess_whisper.py:49-50,75-76)
            rows = [r[: whisper_saved_rows(n, r.shape[1])] for r, n in zip(rows, ticket["lengths"])]
        return rows

    def hold(self, slot: int, futures) -> None:
        self.__dict__.setdefault("_held", {})[slot] = list(futures)

    def _pinned_out(self, slot: int, rows: int, cols: int) -> torch.Tensor:
        for f in self.__dict__.setdefault("_held", {}).pop(slot, []):
            f.result()                                        # writers still reading the buffer we are about to refill
        pool = self.__dict__.setdefault("_pin_out", {})
        buf = pool.get(slot)
        if buf is None or buf.shape[1] != cols or buf.shape[0] < rows:
            buf = torch.empty((max(rows, 1024), cols), dtype=torch.float32).pin_memory()
            pool[slot] = buf
        return buf[:rows]


LAST_RUN: dict = {}       # counters of the most recent _run in this process (bench.py's end-to-end leg reads them)


class _NoDist:
    """``local_only`` runs (bench.py's end-to-end leg at N > 1: every rank extracts ITS OWN directory, weak scaling): the
    driver behaves as a single process -- no sharding, no collective, the caller's process group is left alone."""
    @staticmethod
    def env():
        # "local rank" = the device the caller is already on (bench.py picked it; in a one-GPU gloo rehearsal LOCAL_RANK > 0 is no device)
        return 0, 1, (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    init = staticmethod(lambda *a, **k: None)
    shutdown = staticmethod(lambda: None)
    broadcast_int = staticmethod(lambda v, *a, **k: int(v))
    sum_over_ranks = staticmethod(float)
    max_over_ranks = staticmethod(float)


def _run(argv: Optional[Sequence[str]], whisper: bool, extractor_factory=None, local_only: bool = False) -> int:
    """``extractor_factory(args, whisper, device)`` replaces ``_Extractor`` (bench.py hands in its already-built encoder;
    the CPU gloo tests hand in a stub so that everything around the model call -- sharding, the compat layer index,
    disjoint writes, failure reporting -- runs without a GPU)."""
    from . import dist as D
    if local_only:
        # _Extractor.__init__ talks to the real process group (weight broadcast): a local-only run must bring its own extractor
        assert extractor_factory is not None, "local_only needs an extractor_factory (no collective may run on the caller's group)"
        D = _NoDist
    args = build_parser(whisper).parse_args(argv)
    rank, world, local_rank = D.env()
    average = args.use_average == "y"
    log = print if rank == 0 else (lambda *a, **k: None)
    log(f"Using average = {average}")
    device = f"cuda:{local_rank}" if torch.cuda.is_available() else "cpu"
    log(f"Using device = {'cuda' if torch.cuda.is_available() else 'cpu'}")
    os.makedirs(args.save_path, exist_ok=True)
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
    D.init(device=torch.device("cuda", local_rank) if torch.cuda.is_available() else None)
    # taken once on rank 0 before anybody writes: ranks must not race on len(listdir).  Outputs are written as
    # <name>.tmp and renamed when complete; what a killed run left behind is neither a feature file nor part of the count.
    n_existing = 0
    if rank == 0:
        from .frontend import is_partial, stale_partial
        for fn in os.listdir(args.save_path):
            if is_partial(fn):                      # never a feature file, never counted; removed only when its writer is gone
                if stale_partial(args.save_path, fn):
                    try:
                        os.remove(os.path.join(args.save_path, fn))
                        print(f"Removed stale partial output {fn}")
                    except OSError:
                        pass
            else:
                n_existing += 1
    n_existing = D.broadcast_int(n_existing)
    log(f"Save path = {args.save_path} created. It has {n_existing} files in it.")

    wav_names = os.listdir(args.wav_dir)
    log(f"{len(wav_names)} file are going to be processed...")
    log(f"Checking files in {args.wav_dir}")
    missing = [os.path.join(args.wav_dir, w) for w in wav_names if not os.path.isfile(os.path.join(args.wav_dir, w))]
    if missing:
        log("Missing files:")
        for m in missing:
            log(f" - {m}")
        log("Something went wrong, make sure everything is correct before running again!")
        D.shutdown()
        return 0

    log(f"Extracting features using {args.ssl_type}")
    if device == "cpu" and extractor_factory is None:
        # the product has exactly one backend; say so instead of silently computing elsewhere
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        print("Something went wrong, make sure everything is correct before running again!")
        D.shutdown()
        return 0
    try:
        ex = (extractor_factory or _Extractor)(args, whisper, device)
    except (OSError, NotImplementedError) as e:          # NotImplementedError: a config.json variant the encoders refuse
        log(f"Error: No pretrained model found with the name {args.ssl_type}")
        log(f"  ({e})")
        log("Something went wrong, make sure everything is correct before running again!")
        D.shutdown()
        return 0
    log(f"Weights: {ex.weight_source}; numerics mode {args.mode}")

    num_states = ex.geo.num_layers + 1
    if average:
        layer_index = None
        log("Layer rule: mean of the last four hidden states (--use_average y)")
    elif not whisper and not args.use_n_layer:
        layer_index = n_existing                         # preprocess_speech.py:41,67 (may be out of range -> per-file failure)
        log(f"Layer rule: hidden_states[{n_existing}] = hidden_states[number of files found in --save_path at start-up] "
            f"(the reference's rule, preprocess_speech.py:41,67; --use_n_layer selects hidden_states[--n_layer])")
        if args.skip_existing:
            # resuming under that rule writes the REST of the directory from another layer than the files already there
            log("Error: --skip_existing resumes into a non-empty directory, where the reference's layer rule selects "
                f"hidden_states[{n_existing}] instead of the layer the existing files hold; pass --use_n_layer --n_layer N "
                "(or --use_average y) with --skip_existing")
            log("Something went wrong, make sure everything is correct before running again!")
            D.shutdown()
            return 0
        if n_existing > 0:
            log(f"WARNING: --save_path already holds {n_existing} files, so this run writes hidden_states[{n_existing}] "
                f"of {num_states} (index {num_states - 1} is the last layer); files already present are overwritten by "
                "name, others stay -- a directory can end up holding mixed layers.  Use --use_n_layer --n_layer N to pick the layer.")
    else:
        # an out-of-range --n_layer is what ``hidden_states[N]`` raises per file in the reference (IndexError inside
        # the per-file try/except): keep the raw index and let every file report it, instead of crashing here
        layer_index = args.n_layer if args.n_layer >= 0 else num_states + args.n_layer
        log(f"Layer rule: hidden_states[{args.n_layer}] (--n_layer)")
    bad_layer = layer_index is not None and not 0 <= layer_index < num_states

    # Shard the UNFILTERED, deterministic list first; --skip_existing then filters each rank's own shard.  (Filtering
    # before sharding raced: a fast rank's first .pt files changed the list slower ranks were still about to shard.)
    paths = [os.path.join(args.wav_dir, w) for w in sorted(wav_names)]
    sizes = [os.path.getsize(p) for p in paths]
    mine = shard_files(paths, sizes, rank, world)
    if args.skip_existing:
        ext = ".npy" if args.save_format == "npy" else ".pt"

        def present(p):                                      # outputs are renamed into place when complete; an empty file is not one
            out = feature_path(args.save_path, p)[:-3] + ext
            return os.path.isfile(out) and os.path.getsize(out) > 0
        mine = [p for p in mine if not present(p)]
    batches = make_batches(mine, max(1, args.batch_size))

    # decode into page-locked memory when a GPU is there: the upload is then one async copy per utterance, no packing pass on the
    # launching thread (SER_PINNED_DECODE=0: A/B knob, the round-2 form)
    pinned_decode = torch.cuda.is_available() and os.environ.get("SER_PINNED_DECODE", "1") == "1"

    # --resample: the raw samples go to the GPU at the file's own rate and ser_resample_v runs ahead of the forward (an extractor without
    # upload_resampled -- the stubs of the host tests and tools -- keeps the host filter, as does a rate whose bank would be too large)
    gpu_resample = args.resample and hasattr(ex, "upload_resampled")

    def decode(path):
        """(path, (samples, their rate), None) or (path, None, error)."""
        try:
            if not gpu_resample:
                return path, (load_wav_16k(path, resample=args.resample, pinned=pinned_decode), TARGET_SR), None
            x, sr = decode_wav(path, pinned_decode)
            if sr != TARGET_SR and max(resample_ratio(sr)) > RESAMPLE_MAX_R:
                x, sr = host_resample(x, sr), TARGET_SR
            return path, (x, sr), None
        except Exception as e:                            # noqa: BLE001  (reference: except Exception -> print)
            return path, None, e

    def write(item):
        path, feats = item
        try:
            out = feature_path(args.save_path, path)
            if args.save_format == "npy":
                final = out[:-3] + ".npy"
                from .frontend import tmp_name
                tmp = tmp_name(final)
                with open(tmp, "wb") as f:                   # complete or absent: --skip_existing trusts what it finds
                    np.save(f, feats.numpy())
                os.replace(tmp, final)
            else:
                save_feature(feats, out)
        except Exception as e:                            # noqa: BLE001
            print(f"Failed to process {path}: {e}")

    from tqdm import tqdm
    t0 = time.perf_counter()
    done = 0
    audio_s = 0.0
    bar = tqdm(total=len(mine), desc="Extracting features", disable=(rank != 0))
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        writes = []

        def run(fn, good, **k):
            """fn(waves, layer_index, ...) of (path, (samples, rate)) items; the rates go along only where the GPU resamples."""
            waves = [w for _, (w, _) in good]
            return fn(waves, layer_index, rates=[sr for _, (_, sr) in good], **k) if gpu_resample else fn(waves, layer_index, **k)

        def finished(good, feats, ticket):
            nonlocal done, audio_s
            futs = [pool.submit(write, (path, f)) for (path, _), f in zip(good, feats)]
            writes.extend(futs)
            done += len(good)
            samples = [resampled_len(len(w), sr) for _, (w, sr) in good]
            if ticket is not None:
                ex.hold(ticket["slot"], futs)                 # the slot's pinned buffer is not refilled under its writers
                audio_s += sum(samples) / 16000.0
            else:                                             # through extract: added file by file (the total's last digit
                for n in samples:                             # follows the order of the additions, and SER_RUN rounds it)
                    audio_s += n / 16000.0

        tm = dict(decode_wait=0.0, submit=0.0, finish=0.0)   # where the launching thread spends its time (--timing)
        clock = time.perf_counter

        def submit(good, slot):
            t_a = clock()
            ticket = run(ex.submit, good, slot=slot)
            tm["submit"] += clock() - t_a
            return ticket

        # both encoder families run through the slot pipeline; the contract of a failed batch is batchloop's
        # (an extractor with ``pipelined = False`` has no submit / collect / hold: they are looked up when called)
        pipe = SlotPipeline(submit=submit, collect=lambda ticket: ex.collect(ticket), extract=lambda good: run(ex.extract, good),
                            slots=getattr(ex, "SLOTS", 2), done=finished,
                            fail=lambda item, err: print(f"Failed to process {item[0]}: {err}"),
                            before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None,
                            pipelined=getattr(ex, "pipelined", True))
        decoding = prefetch(batches, pool, decode)           # the next batch is decoded while the GPU works
        for bi in range(len(batches)):
            t_a = clock()
            decoded = next(decoding)
            tm["decode_wait"] += clock() - t_a
            good = []
            for path, item, err in decoded:                   # item: (samples, their rate)
                if err is not None:
                    print(f"Failed to process {path}: {err}")
                else:
                    good.append((path, item))
            if good and bad_layer:
                for path, _ in good:
                    print(f"Failed to process {path}: tuple index out of range")
            elif good:
                pipe.push(bi, good)
            t_a = clock()
            pipe.drain()                                      # all but one slot stay in flight while the next batch is prepared
            tm["finish"] += clock() - t_a
            bar.update(len(decoded))
        pipe.drain(0)
        for w in writes:
            w.result()
    bar.close()
    dt = time.perf_counter() - t0
    total_done, wall = D.sum_over_ranks(done), D.max_over_ranks(dt)
    total_audio = D.sum_over_ranks(audio_s)
    log(f"{int(total_done)} utterances on {world} GPU(s) in {wall:.2f} s ({total_done / max(wall, 1e-9):.1f} utt/s)")
    # one machine-readable line per run (metrics/logging row)
    import json
    log("SER_RUN " + json.dumps({
        "utterances": int(total_done), "audio_s": round(total_audio, 1), "wall_s": round(wall, 3), "n_gpus": world,
        "utt_per_s": round(total_done / max(wall, 1e-9), 1), "audio_s_per_s": round(total_audio / max(wall, 1e-9), 1),
        "mode": args.mode, "ssl_type": args.ssl_type, "batch_size": args.batch_size, "num_workers": args.num_workers,
        "host_cpus": os.cpu_count()}))
    LAST_RUN.clear()
    LAST_RUN.update(done=int(total_done), wall_s=wall, audio_s=total_audio, launch_thread=dict(tm))
    if args.timing:
        log("launch thread: " + ", ".join(f"{k} {v:.3f} s" for k, v in tm.items()) + f", total {dt:.3f} s")
        if getattr(ex, "tm", None):
            log("  submit = " + ", ".join(f"{k} {v:.3f} s" for k, v in ex.tm.items()))
    D.shutdown()
    return 0


# ------------------------------------------------------------------ text extractor (8f-1)
def build_text_parser() -> argparse.ArgumentParser:
    """Flags of the reference's preprocessing/preprocess_roberta.py:12-21, unchanged, + additive ones."""
    from .engine import POST_LN_MODES
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--roberta_type", type=str, default="roberta")
    p.add_argument("--df_path", type=str, default="./")
    p.add_argument("--save_path", type=str, default="./")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--max_len", type=int, default=80, help="tokens per text (at most 512, the models' position range)")
    p.add_argument("--use_average", type=str, default="n")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--mode", type=str, default="f16x", choices=list(POST_LN_MODES),
                   help="numerics: f16x (default: the speech drivers' 3-product split on fp16 hi + lo planes; 5e-6 of the fp32 reference on Gaussian "
                        "weights, 2-5e-5 under sharp attention at 24 layers; values must stay below 65 504 -- checked per batch), fp32x (the same split on "
                        "bf16 planes: fp32 range, 2e-5 / 2-3e-4), bf16 (1e-2)")
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--tokenizer_path", type=str, default="", help="local RobertaTokenizer files (default: --roberta_type)")
    return p


class TextExtractor:
    """``tokenizer(text, padding="max_length", truncation=True, max_length=L)`` -> RoBERTa -> [L, D] per text
    (preprocess_roberta.py:45-76).  ``tokenize`` maps a list of strings to (input_ids, attention_mask) int tensors
    [n, max_len]; the default uses HF's RobertaTokenizer when its files are available locally."""

    def __init__(self, geo, state_dict, device: str, mode: str, tokenize, average: bool):
        from .engine import build_encoder
        self.enc = build_encoder(geo, state_dict, device, mode)      # RoBERTa (TextEncoder) or DeBERTa-v3 (DebertaEncoder)
        self.tokenize, self.average = tokenize, average
        self._range_warned = False

    def extract(self, texts: Sequence[str]) -> List[torch.Tensor]:
        from .engine import mean_last4
        ids, mask = self.tokenize(list(texts))
        hs = self.enc.forward(ids, mask)
        bits = hs.take_range_bits()
        if bits & 1:                                                 # fp16 operand planes saturate: fail the batch instead (speech driver's rule)
            raise ValueError("a value beyond the fp16 operand range of --mode f16x (65504) was met inside the forward: re-run with --mode fp32x")
        if bits & 2 and not self._range_warned:                      # beyond half of it: warn once per run, as the speech driver does
            self._range_warned = True
            print(f"WARNING: values within a factor 2 of the fp16 operand range of --mode {self.enc.mode_name} (65504); "
                  f"--mode fp32x has fp32 range")
        sel = mean_last4(hs) if self.average else hs.states[-1]      # .last_hidden_state
        host = sel.to("cpu")
        return [host[hs.frame_offs[b]: hs.frame_offs[b + 1]] for b in range(len(texts))]


def hf_tokenize_fn(name_or_path: str, max_len: int, family: str = C.FAMILY_ROBERTA):
    """The reference's tokenizer call (preprocess_roberta.py:48-54, preprocess_deroberta.py:48-54 with
    DebertaV2Tokenizer); raises OSError without local files."""
    if family == C.FAMILY_DEBERTA:
        from transformers.models.deberta_v2 import DebertaV2Tokenizer as Tok
    else:
        from transformers import RobertaTokenizer as Tok
    tok = Tok.from_pretrained(name_or_path, local_files_only=True)

    def fn(texts):
        enc = tok(texts, padding="max_length", truncation=True, max_length=max_len, return_tensors="pt")
        return enc["input_ids"], enc["attention_mask"]
    return fn


def run_roberta(argv: Optional[Sequence[str]] = None, tokenize=None, family: str = C.FAMILY_ROBERTA) -> int:
    import pandas as pd
    from . import dist as D
    args = build_text_parser().parse_args(argv)
    rank, world, local_rank = D.env()
    average = args.use_average == "y"
    log = print if rank == 0 else (lambda *a, **k: None)
    log(f"Using average = {average}")
    log(f"Using device = {'cuda' if torch.cuda.is_available() else 'cpu'}")
    os.makedirs(args.save_path, exist_ok=True)
    log(f"Save path = {args.save_path} created. It has {len(os.listdir(args.save_path))} files in it.")
    log(f"Reading dataframe {args.df_path}")
    try:
        df = pd.read_csv(args.df_path)
        texts, names = [str(t) for t in df.transcription.values], [str(n) for n in df.FileName.values]
    except Exception as e:                                # noqa: BLE001 (reference: except Exception -> print)
        log(f"Error reading dataframe from {args.df_path}: {e}")
        log("Something went wrong, make sure everything is correct before running again!")
        return 0
    log(f"Extracting features using {args.roberta_type}")
    if not torch.cuda.is_available():
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        return 0
    torch.cuda.set_device(local_rank)
    D.init(device=torch.device("cuda", local_rank))
    try:
        geo = C.resolve_geometry(args.roberta_type, args.checkpoint)
        if geo.family != family:
            raise OSError(f"{args.roberta_type} is not a {family} encoder")
        if args.max_len > 512:
            raise OSError(f"--max_len {args.max_len}: these text encoders have 512 positions (the reference uses 80)")
        if tokenize is None:
            tokenize = hf_tokenize_fn(args.tokenizer_path or args.roberta_type, args.max_len, family)
        sd, err = None, ""
        if rank == 0:
            try:
                sd, src = find_weights(args.roberta_type, args.checkpoint, args.synthetic_weights, args.seed, geo)
            except OSError as e:
                err = str(e)
        # every rank learns about a failed load BEFORE anybody enters the weight broadcast (the speech driver's rule):
        # otherwise ranks > 0 sit in broadcast_object_list until the collective times out
        if D.broadcast_int(1 if (rank == 0 and sd is None) else 0) == 1:
            raise OSError(err or "rank 0 found no checkpoint")
        sd, _, _ = D.broadcast_state_dict(sd)
        ex = TextExtractor(geo, sd, f"cuda:{local_rank}", args.mode, tokenize, average)
    except OSError as e:
        log(f"Error: No pretrained model found with the name {args.roberta_type}")
        log(f"  ({e})")
        D.shutdown()
        return 0
    mine = list(range(rank, len(texts), world))
    from tqdm import tqdm
    bar = tqdm(total=len(mine), desc="Extracting features", disable=(rank != 0))
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        writes = []
        for idx in make_batches(mine, max(1, args.batch_size)):
            try:
                feats = ex.extract([texts[j] for j in idx])
                for j, f in zip(idx, feats):
                    writes.append(pool.submit(save_feature, f, feature_path(args.save_path, names[j])))
            except Exception as e:                        # noqa: BLE001
                for j in idx:
                    print(f"Failed to process {names[j]}: {e}")
            bar.update(len(idx))
        for w in writes:
            w.result()
    bar.close()
    D.shutdown()
    return 0


def run_deberta(argv: Optional[Sequence[str]] = None, tokenize=None) -> int:
    """preprocessing/preprocess_deroberta.py: the RoBERTa driver with a DeBERTa-v2/v3 checkpoint and tokenizer."""
    return run_roberta(argv, tokenize, family=C.FAMILY_DEBERTA)


def run_speech(argv: Optional[Sequence[str]] = None, extractor_factory=None, local_only: bool = False) -> int:
    return _run(argv, whisper=False, extractor_factory=extractor_factory, local_only=local_only)


def run_whisper(argv: Optional[Sequence[str]] = None, extractor_factory=None, local_only: bool = False) -> int:
    return _run(argv, whisper=True, extractor_factory=extractor_factory, local_only=local_only)
