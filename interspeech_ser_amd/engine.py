"""Host-side encoders: the drop-in for the reference's model call.

The reference does (preprocess_speech.py:49-50,66-67 / preprocess_whisper.py:57,71)

    hidden_states = model(**inputs, output_hidden_states=True).hidden_states
    hidden_states = model.encoder(input_features, output_hidden_states=True).hidden_states

one utterance at a time.  ``SpeechEncoder.forward`` / ``WhisperEncoder.forward``
take a *ragged batch* of raw waveforms and return the same L+1 hidden states for
every utterance, computed entirely by libserhip's gfx950 kernels.  PyTorch is used
for device memory, H2D/D2H copies and the stream handle only.

HBM layout: utterances are packed, never padded -- a batch is one ``[rows, C]``
matrix and ``frame_offs[b]`` is utterance b's first row.  Packed rows make a batched
run arithmetically identical to the reference's batch-of-one loop (no padding frames
exist, so no attention / conv masking is needed) and waste no FLOPs on padding.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .arena import Pinned, SlotArenas, TableBlob
from .weights import check_f16_weight
from .config import (EncoderGeometry, FAMILY_DATA2VEC_AUDIO, FAMILY_ROBERTA, FAMILY_W2V_BERT, FAMILY_W2V_CONFORMER, FAMILY_WAVLM,
                     FAMILY_WHISPER)

MODES = {"bf16": _lib.MODE_BF16, "fp32x": _lib.MODE_FP32X, "f16": _lib.MODE_FP16, "f16q": _lib.MODE_FP16, "f16a": _lib.MODE_FP16,
         "f16x": _lib.MODE_FP16X, "f16m": _lib.MODE_FP16M, "f16mf": _lib.MODE_FP16M}
# "f16mf" (round 5, the drivers' default): "f16m" where it is benign -- FC1 and FC2 (2/3 of the layer FLOPs) in every layer, the packed
# projection from a third of the depth on (_EncoderBase.qkv_m_from, _lay_modes); the conv stem, ser_attention, the output projection and
# the first third's packed projections keep "f16x"'s three products on fp16 hi + lo planes.  oracle/numerics_whatif_f16m.py (site lists): under sharp
# attention the error of "f16m" comes from the packed projections of the FIRST layers (an error injected by layer i passes through L - i
# more softmax layers): all of them 4.3e-4 of f16m's 5.2e-4 at 24 layers, from layer 8 on nothing measurable; FC1 + FC2 alone give 1.4e-4
# (sharp x2), 2.7e-5 (LoRA), 1.3e-5 (plain) -- inside "fp32x"'s on each.  The stem in that format: 1.4e-3 (it stays on 22 bits).
# "f16m" (round 5): the encoder layers' GEMMs on SER_MODE_FP16M operands -- fp16 main product + block-scaled e4m3 cross terms on gfx950's
# v_mfma_scale_f32_16x16x128_f8f6f4: 2 product-equivalents per algorithmic FLOP instead of "f16x"'s 3 (include/ser_hip.h).  The packed
# projection, FC1 and FC2 multiply in it (opt-in, SER_F16M_OUT_M=1, head dim 64: the output projection too, on FP16M context rows out of
# ser_attention, ABI 14); ser_attention, the output projection and the conv stem stay on fp16 hi + lo planes.  Operand error ~2^-15 (between "f16"'s 2^-11 and
# "f16x"'s 2^-22): oracle/numerics_whatif_f16m.py, tests/test_gpu_depth.py.
# "f16x" (round 4): the 3-product split EVERYWHERE, like "fp32x", on fp16 hi + lo planes -- 22-bit operands instead of the 16 of the
# bf16 pair at the same cost.  The widest margin of all modes where |values| stay inside fp16's range (65 504).
# "f16": encoder layers on single-product fp16 operands (11 significand bits at the bf16 MFMA rate), the convolutional
# stem -- where operand rounding hurts most and only 13 % of the FLOPs live -- on the 3-product FP32X split.
# "f16q": "f16" with the LOGIT path of every layer fp32-grade: the q / k (+ WavLM gate) columns of the packed projection and
# S = K Q^T inside the attention kernel run the 3-product split on fp16 hi + lo planes (SER_MODE_FP16X), v / P V / output
# projection / feed-forward stay single-product fp16.  A softmax weight moves by (logit error) * ln 2, so q / k rounding is
# what sharp attention maps (trained checkpoints, LoRA-scaled query projections) amplify; ~19 % of the layer FLOPs pay 3x.
# "f16a": the whole ATTENTION BLOCK of every layer (packed projection, attention, output projection) on the fp16 hi + lo split,
# the feed-forward pair (62 % of the layer FLOPs) on single fp16 products.  oracle/numerics_whatif.py: under sharp attention the
# error comes from the attention block as a whole -- rounding v, P, the context rows or the output-projection weights once is
# amplified by the following layers' softmax as much as rounding q and k -- while the feed-forward rounding is benign.
# The modes of the post-LayerNorm encoders (RoBERTa, DeBERTa, the *-base speech encoders; f16x first: the text drivers' default).  The
# others would need an FP16M operand copy out of ser_layernorm, which runs between their GEMMs.
POST_LN_MODES = ("f16x", "fp32x", "bf16")
_PLANES = {_lib.MODE_BF16: 1, _lib.MODE_FP32X: 2, _lib.MODE_FP16: 1, _lib.MODE_FP16X: 2, _lib.MODE_FP16M: 2}
_DTYPE = {_lib.MODE_BF16: torch.bfloat16, _lib.MODE_FP32X: torch.bfloat16, _lib.MODE_FP16: torch.float16,
          _lib.MODE_FP16X: torch.float16, _lib.MODE_FP16M: torch.float16}
# MFMA products per algorithmic FLOP of a GEMM launch in each operand format (FP16M: the scaled e4m3 instruction runs at twice the fp16 rate)
_PRODUCTS = {_lib.MODE_BF16: 1, _lib.MODE_FP32X: 3, _lib.MODE_FP16: 1, _lib.MODE_FP16X: 3, _lib.MODE_FP16M: 2}


# A/B knob (tools/): SER_NO_SHIFT=1 turns the shifted operand copy of the encoder layers off (state 0 is still centred)
import os as _os
_NO_SHIFT = _os.environ.get("SER_NO_SHIFT", "0") == "1"
# (Round 3's SER_SPLIT_GATE -- the 2H gate columns as their own narrow launch -- measured -0.3 % and was removed in round 4: DESIGN.md section 10.)
# WavLM's gate pre-activations: computed by ser_attention from the layer input's operand copy (ser_attention_args.gate_x; default), or
# 2H extra columns of the packed projection (SER_GATE_IN_ATTN=0, rounds 1-3: a 13th 256-wide column tile for 32 columns).  Measured on the
# step (tools/gate_in_attn_ab.sh, two A/B pairs per build, one box; profiles/r03_gate_in_attn_ab.txt): bf16 2 018 / 2 018 -> 2 029 / 2 029
# utt/s, f16a 1 134 / 1 135 -> 1 154 / 1 159 (there the 13th tile column is a 3-product one).  The first form of the kernel side guarded its
# loads (a branch and a vmcnt(0) each in hipcc's output) and LOST 0.4 % in bf16: the prologue of ser_attention is latency-bound.
# (Read when an encoder is built: _EncoderBase.gate_in_attn.)
# A/B knob: SER_STEM_F16X=0 puts the stem of the f16 / f16q / f16a modes back on bf16 hi + lo planes (rounds 2 / early 3)
_STEM_F16X = _os.environ.get("SER_STEM_F16X", "1") == "1"


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Sz(int):
    """A per-batch size (row count, utterances, longest utterance) that remembers its name.  It is an ``int`` everywhere;
    a launch recorded into a command list keeps the name so the field can be patched for the next batch."""

    def __new__(cls, value: int, name: str):
        o = int.__new__(cls, value)
        o.name = name
        return o


class Tape:
    """The launches of one forward over a slot's arena, recorded as ``ser_cmd`` entries (include/ser_hip.h).  Pointers
    in an arena never change, so a later batch only patches its sizes (``Sz`` fields) and replays everything with one
    ``ser_run`` call: ~150 Python -> C transitions per batch become one."""

    def __init__(self, capacity: int = 640):
        self.cmds = (_lib.Cmd * capacity)()
        self.n = 0
        self.patches = []                    # (struct view inside cmds, field name, size name)
        self.inputs: List[tuple] = []        # (struct view inside cmds, field name) of every launch that reads the per-batch waveform
        self.marks: Dict[int, int] = {}      # hidden state index -> number of leading commands that produce states[0..index]
        self.parts: List[tuple] = []         # (name, number of leading commands) where a recorder marks the end of a part (tools/codec_bench.py)
        self.over: tuple = ()                # the dicts beyond its keeper's that the recorded pointers lie in (_LaunchHost._replay)
        self._failed = C.c_int32(-1)

    def slot(self, union_field: str):
        if self.n >= len(self.cmds):
            raise _lib.SerHipError("command list capacity exceeded")
        return getattr(self.cmds[self.n].u, union_field)

    def commit(self, op: int, view, **sizes) -> None:
        self.cmds[self.n].op = op
        for field, value in sizes.items():
            if isinstance(value, Sz):
                self.patches.append((view, field, value.name))
        self.n += 1

    def subset(self, keep, by_cmd: bool = False) -> "Tape":
        """Measurement aid (bench.py ``step_decomposition``): a command list holding copies of the recorded launches whose op
        satisfies ``keep(op)`` (or, with ``by_cmd``, ``keep(cmd)``: two uses of one op apart), with the sizes of the batch that ran last.  Same pointers, same shapes, same kernels -- replayed
        on its own it shows what ONE class of kernels (the GEMMs, the attention kernels, the row kernels) costs in the regime
        the step runs them in (two utterance groups on parallel graph branches)."""
        picked = [i for i in range(self.n) if keep(self.cmds[i] if by_cmd else self.cmds[i].op)]
        t = Tape(max(1, len(picked)))
        for j, i in enumerate(picked):
            C.memmove(C.byref(t.cmds[j]), C.byref(self.cmds[i]), C.sizeof(_lib.Cmd))
        t.n = len(picked)
        return t

    def run(self, sizes: Dict[str, int], stream: int, last_state: Optional[int] = None, wave: Optional[int] = None) -> None:
        """Replay the list with this batch's ``sizes`` and waveform (``wave``: its device address); with ``last_state`` only the leading
        commands that produce hidden states 0..last_state."""
        for view, field, name in self.patches:
            setattr(view, field, sizes[name])
        if wave is not None:
            for view, field in self.inputs:
                setattr(view, field, wave)
        n = self.n if last_state is None else self.marks.get(last_state, self.n)
        rc = lib.ser_run(self.cmds, n, C.byref(self._failed), stream)
        if rc != 0:
            check(rc, f"ser_run (command {self._failed.value} of {n})")


def _on_stream(fn):
    """Look the launch stream up once for the whole forward (see ``_EncoderBase._s``)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        prev = self._st
        self._st = _stream()
        try:
            return fn(self, *a, **k)
        finally:
            self._st = prev
    return wrapped


class Act:
    """16-bit GEMM operand with 1 (bf16 / fp16) or 2 (bf16 hi/lo) planes: tensor [planes, rows, cols]."""

    def __init__(self, rows: int, cols: int, planes: int, device, zero: bool = False, extra_rows: int = 0,
                 dtype=torch.bfloat16, mx: bool = False):
        alloc = torch.zeros if zero else torch.empty
        self.t = alloc((planes, rows + extra_rows, cols), dtype=dtype, device=device)
        self.rows, self.cols, self.planes = rows, cols, planes
        self.plane_stride = (rows + extra_rows) * cols
        # SER_MODE_FP16M: plane 1 holds the e4m3 cross-term bytes; one uint32 of four block-scale codes per (64-column tile, row)
        self.scale = torch.zeros((cols // 64, rows + extra_rows), dtype=torch.int32, device=device) if mx else None
        self.scale_ld = rows + extra_rows

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def first_rows(self, rows: int) -> "Act":
        """The first ``rows`` rows of every plane as an operand of their own: same storage, same plane stride."""
        v = copy.copy(self)
        v.rows = rows
        return v

    def float(self) -> torch.Tensor:
        """fp32 view for tests (hi + lo)."""
        if self.scale is not None:
            raise NotImplementedError("FP16M tensors: plane 1 is not a 16-bit lo plane")
        return self.t[:, : self.rows].float().sum(dim=0)


@dataclass
class Linear:
    w: torch.Tensor            # [planes, N, K] bf16
    b: Optional[torch.Tensor]  # [N] fp32
    N: int
    K: int
    colsum: Optional[torch.Tensor] = None   # [N] fp32: sum_k of the stored (gamma-folded) planes, deferred LayerNorm
    wscale: Optional[torch.Tensor] = None   # SER_MODE_FP16M: [K / 64, N] int32 block-scale words


class HiddenStates:
    """What ``.hidden_states`` is in the reference: L+1 states per utterance.
    ``states`` is one fp32 tensor [L+1, rows, D]; utterance b owns rows
    frame_offs[b]:frame_offs[b+1] (crop to the true frame count is implicit)."""

    def __init__(self, states: torch.Tensor, frame_offs: Sequence[int], computed: Optional[int] = None,
                 range_flag: Optional[torch.Tensor] = None, frame_offs_dev: Optional[torch.Tensor] = None):
        self.states = states
        self.frame_offs = list(int(x) for x in frame_offs)
        # the same offsets as int32 [B + 1] on the device, where the forward's plan keeps them (valid until the slot's next plan): what a
        # consumer that stays on the device reads (PoolHead)
        self.frame_offs_dev = frame_offs_dev
        # states[0 .. computed-1] hold this batch's results; a forward stopped early (``last_state``) leaves the rest stale
        self.computed = states.shape[0] if computed is None else int(computed)
        self.range_flag = range_flag

    def __len__(self) -> int:
        return self.states.shape[0]

    @property
    def batch(self) -> int:
        return len(self.frame_offs) - 1

    def utterance(self, b: int, layer: int) -> torch.Tensor:
        idx = layer if layer >= 0 else layer + self.states.shape[0]
        if not 0 <= idx < self.computed:
            raise IndexError(f"hidden state {layer} is not available (states 0..{self.computed - 1} were computed)")
        return self.states[idx, self.frame_offs[b]: self.frame_offs[b + 1]]

    def frames(self, b: int) -> int:
        return self.frame_offs[b + 1] - self.frame_offs[b]

    # fp16 range guard (round 5): every kernel that rounds a value to an fp16 operand plane (GEMM / row-kernel epilogues in the f16x, f16m,
    # f16a, f16q, f16 modes) ORs into the slot's device word -- bit 0: a value beyond +-65504 (it saturated), bit 1: beyond half of that.
    # ``range_flag`` is that word (int32 [1] on the device, None in the bf16-plane modes); the caller reads it back with the features
    # and clears it (``take_range_bits``).  Round 4 reduced max|hidden state| with a torch pass on sampled batches only.

    def take_range_bits(self, pinned_out: Optional[torch.Tensor] = None):
        """Enqueue (current stream) the read-back of the guard word into ``pinned_out`` (int32 [1], page-locked) and its reset; with no
        buffer given: synchronous, returns the bits.  0 in the modes that keep no fp16 planes."""
        if self.range_flag is None:
            if pinned_out is not None:
                pinned_out.zero_()
            return 0
        if pinned_out is not None:
            pinned_out.copy_(self.range_flag, non_blocking=True)
            self.range_flag.zero_()
            return None
        bits = int(self.range_flag.item())
        self.range_flag.zero_()
        return bits


def _operand_mode(mode_name: str) -> int:
    """GEMM operand format of the heads: bf16 in mode "bf16", bf16 hi + lo in "fp32x", fp16 hi + lo in every other mode -- their products
    feed a softmax over the frames, where single-product rounding is not benign"""
    return {"bf16": _lib.MODE_BF16, "fp32x": _lib.MODE_FP32X}.get(mode_name, _lib.MODE_FP16X)


class _LaunchHost:
    """Weight and launch helpers (``_linear`` / ``_dev_f32`` / ``_gemm`` / ``_layernorm``) and the one record-or-replay path (``_replay``):
    the base of every encoder, and used as it is by the fusion heads -- one operand format for every GEMM, launches issued at once
    (nothing is recorded)."""

    use_tape = True          # replay recorded command lists (one foreign call per forward); False = launch one by one

    def __init__(self, device, mode_name: str, mode: int, stem_mode: int, fp16_planes: bool):
        if not torch.cuda.is_available():
            raise _lib.SerHipError("no HIP device visible: the extraction path has no CPU fallback")
        self.device = torch.device(device)
        self.mode_name = mode_name
        self.mode, self.stem_mode = mode, stem_mode              # operand format of the layers' GEMMs / of the stem's
        self.fp16_planes = fp16_planes                           # operand copies with fp16's range: the guard word is live
        self.geo: Optional[EncoderGeometry] = None               # an encoder's geometry; without one, _layernorm needs its ``eps``
        # when a list, every ser_gemm launch appends (start_event, end_event, algorithmic_flops):
        # bench.py uses it for the live roofline figure of the dominant kernel
        self.gemm_trace: Optional[list] = None
        # when a list, every encoder layer appends (start_event, end_event, utterances) around its attention block
        # (packed QKV projection -> attention -> output projection): bench.py's "attention_block" figure
        self.block_trace: Optional[list] = None
        self._flag: Optional[int] = None    # device address of the range-guard word of the slot being launched / recorded
        self._st: Optional[int] = None      # launch stream of the forward in progress (looked up once per forward)
        self._rec: Optional[Tape] = None    # when set, _issue records the launch helpers' commands into it instead of launching them

    def _s(self) -> int:
        """HIP stream of the current forward: torch.cuda.current_stream() costs ~15 us and a forward makes ~150 launches."""
        return self._st if self._st is not None else _stream()

    # ------------------------------------------------------------------ weights
    def _dev_f32(self, t: torch.Tensor) -> torch.Tensor:
        """fp32 copy on the device that the encoder OWNS: a state dict that arrived by broadcast is made of views into one flat
        bucket in HBM (dist.broadcast_state_dict); keeping such a view would pin the whole fp32 checkpoint (1.3 GB WavLM-large,
        8.6 GB XLS-R-2B) beside the 16-bit planes for the life of the run, and its start is only 4-byte aligned."""
        return t.detach().to(device=self.device, dtype=torch.float32, copy=True).contiguous()

    def _linear(self, w: torch.Tensor, b: Optional[torch.Tensor], stem: bool = False, mode: Optional[int] = None,
                name: str = "a weight") -> Linear:
        """fp32 [N, K] -> 16-bit operand planes on the device (ser_split_bf16): bf16 hi (+ lo), or fp16 (hi + lo for FP16X).
        fp16 planes refuse a weight they cannot hold (weights.check_f16_weight, ValueError naming ``name``)."""
        w = w.detach().to(torch.float32).contiguous()
        N, K = w.shape
        if mode is None:
            mode = self.stem_mode if stem else self.mode
        if mode in (_lib.MODE_FP16, _lib.MODE_FP16X, _lib.MODE_FP16M):
            # on the host, on the exact fp32 tensor split below; ser_pack_f16m's range_flag would see the same values, so its weight
            # launch passes none
            check_f16_weight(w, name)
        src = w.to(self.device)
        out = torch.empty((_PLANES[mode], N, K), dtype=_DTYPE[mode], device=self.device)
        if mode == _lib.MODE_FP16M:
            if K % 64:
                raise ValueError(f"FP16M weights need K % 64 == 0 (K = {K})")
            wscale = torch.zeros((K // 64, N), dtype=torch.int32, device=self.device)
            check(lib.ser_pack_f16m(src.data_ptr(), K, N, K, out.data_ptr(), K, N * K, wscale.data_ptr(), N, 1, None, _stream()), "ser_pack_f16m")
            torch.cuda.current_stream().synchronize()
            return Linear(out, None if b is None else self._dev_f32(b), N, K, wscale=wscale)
        check(lib.ser_split_bf16(src.data_ptr(), out.data_ptr(), N * K, mode, N * K, _stream()), "ser_split_bf16")
        torch.cuda.current_stream().synchronize()
        return Linear(out, None if b is None else self._dev_f32(b), N, K)

    def _linear_ln(self, w: torch.Tensor, b: Optional[torch.Tensor], ln_w: torch.Tensor, ln_b: torch.Tensor,
                   mode: Optional[int] = None, name: str = "a weight") -> Linear:
        """Linear that consumes LayerNorm(x) given the RAW x (deferred LayerNorm, ser_hip.h):
        store W' = W * gamma, colsum(W') of exactly the bf16 planes the MFMAs will read, and
        t = beta W^T + b.  Load-time transform, like the weight-norm fold."""
        w64, g64, be64 = w.detach().double(), ln_w.detach().double(), ln_b.detach().double()
        lin = self._linear((w64 * g64[None, :]).float(), None, mode=mode, name=f"{name} (folded with its LayerNorm weight)")
        t = w64 @ be64
        if b is not None:
            t = t + b.detach().double()
        lin.b = self._dev_f32(t.float())
        if lin.wscale is not None:          # FP16M: the effective weight is w_hi + (the e4m3 image of) w_lo = the fp32 fold to ~2^-15
            lin.colsum = self._dev_f32((w64 * g64[None, :]).float().double().sum(dim=1).float())
        else:
            lin.colsum = lin.w.double().sum(dim=(0, 2)).float().contiguous()
        return lin

    def _new_act(self, rows, cols, zero=False, extra_rows=0, stem=False, mode: Optional[int] = None) -> Act:
        if mode is None:
            mode = self.stem_mode if stem else self.mode
        return Act(rows, cols, _PLANES[mode], self.device, zero=zero, extra_rows=extra_rows, dtype=_DTYPE[mode], mx=(mode == _lib.MODE_FP16M))

    # ------------------------------------------------------------------ launchers
    # Every helper builds its launch once, as a ``ser_cmd``: recording and launching differ in WHEN it goes to the library, not in how it is built.
    def _cmd(self, field: str):
        """The zeroed argument struct (``ser_cmd`` union member) to fill: the command list's next slot when recording, else the member of
        a fresh ``ser_cmd`` -- one per launch: the helpers rely on the zeros, and host threads share nothing."""
        if self._rec is not None:
            return self._rec.slot(field)
        cmd = _lib.Cmd()
        view = getattr(cmd.u, field)
        view.cmd = cmd                      # a Python attribute, not a field: how _issue finds the command around ``view``
        return view

    def _issue(self, op: int, view, what: str, input: Optional[str] = None, **sizes) -> None:
        """Recording: commit the filled command (``Sz`` sizes become patches, ``input`` names the field of ``view`` that takes the
        per-batch waveform pointer); else launch it now, alone, through the dispatcher the list goes through."""
        rec = self._rec
        if rec is not None:
            if input is not None:
                rec.inputs.append((view, input))
            rec.commit(op, view, **sizes)
            return
        view.cmd.op = op
        check(lib.ser_run(C.byref(view.cmd), 1, None, self._s()), what)

    # ------------------------------------------------------------------ record once, then patch and replay
    @contextlib.contextmanager
    def _launching(self, tape: Optional[Tape], hosts: Sequence["_LaunchHost"] = ()):
        """Inside, this host and ``hosts`` (further hosts whose helpers the same forward calls) issue on this host's stream with its
        guard word: into ``tape`` when one is given, else at once."""
        hosts = (self,) + tuple(hosts)
        saved = [(h._rec, h._st, h._flag) for h in hosts]
        for h in hosts:
            h._rec, h._st, h._flag = tape, self._st, self._flag
        try:
            yield
        finally:
            for h, old in zip(hosts, saved):
                h._rec, h._st, h._flag = old

    def _replay(self, owners: Sequence[dict], sizes: Dict[str, int], launch, wave: Optional[int] = None,
                last_state: Optional[int] = None, hosts: Sequence["_LaunchHost"] = ()) -> None:
        """One forward of ``launch(last_state)``.  Launched one by one when ``use_tape`` is off or a trace list is set; else the command
        list kept in ``owners[0]["tape"]`` is replayed with this batch's ``sizes`` and waveform address, and ``launch(None)`` records it
        first (launching nothing) when there is none yet.  ``owners``: the arena / plan dicts the launches' pointers lie in.  A list is
        valid only over the very dicts it was recorded over: a grown arena is a new dict (arena.SlotArenas) and so has none, and one
        that also points into another host's arena (``owners[1:]``) is recorded again when that arena was replaced."""
        if not self.use_tape or self.gemm_trace is not None or self.block_trace is not None:
            with self._launching(None, hosts):
                launch(last_state)
            return
        tape, rest = owners[0].get("tape"), tuple(owners[1:])
        if tape is None or len(tape.over) != len(rest) or any(a is not b for a, b in zip(tape.over, rest)):
            tape = Tape()
            with self._launching(tape, hosts):
                launch(None)
            tape.over = rest
            owners[0]["tape"] = tape
        tape.run(sizes, self._s(), last_state, wave=wave)

    def recorded_tape(self, lengths: Sequence[int], slot: int) -> Tape:
        """the command list the slot's last forward over ``lengths`` replayed (kept per arena; Whisper encoder and decoder: per plan)"""
        pl = self._plan(lengths, slot)
        arenas = getattr(self, "_arenas", None)
        tape = (pl if arenas is None else arenas[slot]).get("tape")
        if tape is None:
            raise _lib.SerHipError("no recorded command list for this slot yet (run a forward first)")
        return tape

    def _gemm(self, a: Act, lin: Linear, M: int, *, a_rowoff=None, lda=None, kc=0, ldj=0, groups=1,
              a_group_stride=0, w_group_stride=0, c_group_stride=0, N=None, K=None, act=_lib.ACT_NONE,
              residual=None, ldr=0, res_row_mod=0, out_f32=None, ldo_f32=0, out_act: Optional[Act] = None,
              out_rowmap=None, a_ptr_offset=0, k_algo=None, ln=None, ln_eps=1e-5, tile_cfg=0,
              ln_stats=None, ln_groups=0, stat_out=None, stat_groups=0, f32_col_begin=0,
              col_scale=1.0, col_scale_end=0, shift=None, ln_mean=None, stem=False, out_mode=0, mode=None, out_col=0,
              lnstat_out=None, gn=None):
        g = self._cmd("gemm")
        g.A = a.ptr + a_ptr_offset
        g.a_plane_stride = a.plane_stride
        g.a_rowoff = _ptr(a_rowoff)
        g.lda = a.cols if lda is None else lda
        g.kc, g.ldj = kc, ldj
        g.W = lin.w.data_ptr()
        g.w_plane_stride = lin.w.shape[1] * lin.w.shape[2]
        g.M, g.N, g.K = M, (lin.N if N is None else N), (lin.K if K is None else K)
        g.groups = groups
        g.a_group_stride, g.w_group_stride, g.c_group_stride = a_group_stride, w_group_stride, c_group_stride
        g.mode = mode if mode is not None else (self.stem_mode if stem else self.mode)
        g.out_mode = out_mode if out_mode != g.mode else 0
        g.bias = _ptr(lin.b)
        g.act = act
        g.residual = _ptr(residual)
        g.ldr = ldr
        g.res_row_mod = res_row_mod
        g.out_f32 = _ptr(out_f32)
        g.ldo_f32 = ldo_f32
        g.out_act = None if out_act is None else out_act.ptr + 2 * out_col     # out_col: first column written (16-bit elements)
        g.ldo_act = 0 if out_act is None else out_act.cols
        g.out_plane_stride = 0 if out_act is None else out_act.plane_stride
        g.out_rowmap = _ptr(out_rowmap)
        if ln is not None:                      # fused LayerNorm over the output row (conv stack)
            g.ln_gamma, g.ln_beta, g.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), float(ln_eps)
        g.tile_cfg = tile_cfg
        if ln_stats is not None:                # deferred LayerNorm of the A rows
            g.ln_stats_in, g.ln_groups, g.ln_colsum = ln_stats.data_ptr(), ln_groups, lin.colsum.data_ptr()
            g.ln_eps = float(self.geo.layer_norm_eps)
        if stat_out is not None:
            g.stat_out, g.stat_groups = stat_out.data_ptr(), stat_groups
        g.f32_col_begin = f32_col_begin
        g.col_scale, g.col_scale_end = float(col_scale), int(col_scale_end)
        if shift is not None:                   # producer side of the shifted operand copy (ser_hip.h): (mean of residual, shift_out, const)
            s_in, s_out, s_const = shift
            g.shift_in, g.shift_out, g.shift_const = _ptr(s_in), s_out.data_ptr(), float(s_const)
        if ln_mean is not None:                 # consumer side: (shift of the A rows, absolute row mean out)
            g.ln_shift, g.mean_out = _ptr(ln_mean[0]), ln_mean[1].data_ptr()
        g.lnstat_out = _ptr(lnstat_out)         # (relative mean, rstd) of the A rows for the attention kernel's in-kernel gate
        g.range_flag = self._flag if out_act is not None else None
        if gn is not None:                      # GroupNorm-over-time stem: (scale, shift, row offsets, B) -- per-(utterance, column) affine
            g.gn_scale, g.gn_shift, g.gn_row_offs, g.gn_B, g.gn_ld = gn[0].data_ptr(), gn[1].data_ptr(), gn[2].data_ptr(), gn[3], gn[0].shape[1]
        if g.mode == _lib.MODE_FP16M:           # block scales of both operands
            g.a_scale, g.a_scale_ld = a.scale.data_ptr(), a.scale_ld
            g.w_scale, g.w_scale_ld = lin.wscale.data_ptr(), lin.wscale.shape[1]
        if out_act is not None and (g.out_mode or g.mode) == _lib.MODE_FP16M:
            if out_col % 64:
                raise ValueError("an FP16M output must start on a 64-column tile")
            g.out_scale, g.out_scale_ld = out_act.scale.data_ptr() + 4 * (out_col // 64) * out_act.scale_ld, out_act.scale_ld
        trace = self.gemm_trace                 # (never on while a list is recorded: _replay)
        if trace is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        self._issue(_lib.OP_GEMM, g, "ser_gemm", M=M, **({} if gn is None else {"gn_B": gn[3]}))
        if trace is None:
            return
        e1.record()
        # algorithmic FLOPs: 2*M*N*K over real (unpadded) channels, no tile-padding FLOPs
        k_real = g.K if k_algo is None else k_algo
        # algorithmic HBM bytes: every operand / result element touched exactly once
        planes = _PLANES[g.mode]
        nbytes = 2.0 * planes * (M * k_real * groups + g.N * groups * k_real)
        nbytes += 4.0 * M * g.N * groups * ((residual is not None) + (out_f32 is not None))
        nbytes += 2.0 * planes * M * g.N * groups * (out_act is not None)
        trace.append((e0, e1, 2.0 * M * g.N * groups * k_real, nbytes, _PRODUCTS[g.mode]))

    def _layernorm(self, x: torch.Tensor, ldx: int, ln, rows: int, D: int, *, gelu=False, out_f32=None,
                   out_act: Optional[Act] = None, eps=None, stem=False, ldo_f32: Optional[int] = None):
        """``ldo_f32``: pitch of ``out_f32`` when its rows are a column block of a wider buffer (default: D)"""
        g, b = ln
        mode = self.stem_mode if stem else self.mode
        if mode == _lib.MODE_FP16M:                   # ser_layernorm writes no FP16M copy; the encoders only need its fp32 output in that mode
            if out_act is not None:
                raise NotImplementedError("ser_layernorm has no FP16M operand copy")
            mode = _lib.MODE_FP16X
        eps = float(self.geo.layer_norm_eps if eps is None else eps)
        o_act = None if out_act is None else out_act.ptr
        ldo_act = 0 if out_act is None else out_act.cols
        ops = 0 if out_act is None else out_act.plane_stride
        ldo_f32 = (D if ldo_f32 is None else ldo_f32) if out_f32 is not None else 0
        a = self._cmd("layernorm")
        a.x, a.ldx, a.g, a.b, a.eps, a.gelu = x.data_ptr(), ldx, g.data_ptr(), b.data_ptr(), eps, int(gelu)
        a.out_f32, a.ldo_f32, a.out_act, a.ldo_act, a.out_plane_stride = _ptr(out_f32), ldo_f32, o_act, ldo_act, ops
        a.mode, a.rows, a.D = mode, rows, D
        a.range_flag = self._flag if out_act is not None else None
        self._issue(_lib.OP_LAYERNORM, a, "ser_layernorm", rows=rows)


class _EncoderBase(_LaunchHost):
    def __init__(self, geo: EncoderGeometry, device, mode: str, post_ln: bool = False):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {list(MODES)}")
        if post_ln and mode not in POST_LN_MODES:
            raise ValueError(f"the post-LayerNorm encoders support the {', '.join(POST_LN_MODES)} numerics modes")
        self.post_ln = post_ln
        # conv stem (+ projection, positional conv): the 3-product split in every parity mode.  The fp16-layer modes take it on fp16 hi + lo
        # planes (22-bit operands, round 3) rather than bf16 hi + lo (16-bit, the "fp32x" mode's): same cost, and the stem's share of the error
        # -- which sharp attention amplifies like any other -- drops by the 6 extra bits per operand
        stem_mode = (_lib.MODE_FP16X if _STEM_F16X else _lib.MODE_FP32X) if mode in ("f16", "f16q", "f16a") else MODES[mode]
        if mode in ("f16m", "f16mf"):
            stem_mode = _lib.MODE_FP16X
        # operand copies with fp16's range: the guard word is live (SER_NO_RANGE_GUARD=1: A/B knob for tools/, never the drivers)
        fp16_planes = mode in ("f16x", "f16m", "f16mf", "f16a", "f16q", "f16") and _os.environ.get("SER_NO_RANGE_GUARD", "0") != "1"
        super().__init__(device, mode, MODES[mode], stem_mode, fp16_planes)
        self.geo = geo
        # WavLM gate inside ser_attention (see the note at the top) -- except beside a packed projection in SER_MODE_FP16M, where it rides as 2H
        # extra output columns (per layer: _lay_modes)
        self.gate_in_attn = _os.environ.get("SER_GATE_IN_ATTN", "1") == "1"
        self.qk_mode = _lib.MODE_FP16X if mode == "f16q" else None             # logit path on its own launch (None: one packed launch)
        self.attn_mode = _lib.MODE_FP16X if mode in ("f16a", "f16m", "f16mf") else self.mode   # attention kernel, context rows, output projection
        self.qkv_mode = self.attn_mode                                         # packed projection (layers before qkv_m_from)
        self.x_mode = self.qk_mode or self.qkv_mode                            # format of the operand copy the packed projection reads
        self.qkv_out_mode = self.x_mode                                        # format of q, k, v (what ser_attention reads)
        # First layer whose PACKED PROJECTION multiplies in SER_MODE_FP16M (see _lay_modes): "f16m" 0 = every layer; "f16mf" a third of the
        # depth (8 of 24, 16 of 48, 11 of 32).  An operand error injected by layer i passes through L - i more softmax layers: the what-if
        # (oracle/numerics_whatif_f16m.py, sites "qkv>=N") puts the packed projection in that format from layer 8 of 24 on at 1.44e-4 / 3.7e-5
        # (sharp x2 / LoRA) against 1.43e-4 / 2.7e-5 with none and 5.2e-4 / 4.7e-4 with all -- its error lives in the first layers.
        self.qkv_m_from: Optional[int] = {"f16m": 0, "f16mf": (geo.num_layers + 2) // 3}.get(mode)
        if mode == "f16mf" and _os.environ.get("SER_F16MF_QKV_FROM"):          # A/B knob (tools/): -1 = never
            v = int(_os.environ["SER_F16MF_QKV_FROM"])
            self.qkv_m_from = None if v < 0 else v
        self.planes, self.stem_planes = _PLANES[self.mode], _PLANES[self.stem_mode]
        self._cache: Dict = {}

    def _guard_word(self, pl) -> Optional[torch.Tensor]:
        """the slot's range-guard word (allocated with the plan); launch helpers pick its address up from ``self._flag``"""
        if not self.fp16_planes:
            self._flag = None
            return None
        t = pl.get("range_flag")
        if t is None:
            t = pl["range_flag"] = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._flag = t.data_ptr()
        return t

    def _lay_modes(self, i: int) -> dict:
        """Formats around layer i's packed projection: the GEMM's mode, the layer input's operand copy it reads (written by ser_row_center for
        layer 0, by FC2 of layer i - 1 otherwise), q / k / v as ser_attention reads them, and where the WavLM gate is evaluated.  With the
        projection in SER_MODE_FP16M the gate rides as 2H extra output columns: the in-kernel form multiplies the layer input's operand copy,
        whose second plane is e4m3 bytes in that format."""
        if self.qkv_m_from is not None and i >= self.qkv_m_from:
            # ... and with head dim 64 (a head = one 64-column tile) ser_attention can write its context rows as FP16M operands (ABI 14), so that
            # the OUTPUT projection of these layers multiplies in the format too (what-if "qkv>=8+out>=8": 1.44e-4 / 4.1e-5; + 1.6 % on the
            # default's step, same envelope on WavLM-large).  OPT-IN (SER_F16M_OUT_M=1), not the default (a performance decision of its own).
            # Its 0.57 on bench.py's Whisper-large-v3 record was not the format: the FP16M output projections filled every 64-column slot of the
            # row partials ``ph``, the 3-product output projection of the first layers (256 x 256 tile, 128-column waves) wrote only every
            # other slot, and from the second forward over a plan on the first layers' LayerNorm summed the stale ones.  ser_gemm now zeroes
            # the second slot of such a wave (tests/test_gpu_replay.py, test_gpu_kernels.py: stat_out slots).
            return dict(qkv_mode=_lib.MODE_FP16M, x_mode=_lib.MODE_FP16M, qkv_out_mode=self.attn_mode, gate_in_attn=False,
                        out_m=self.geo.head_dim == 64 and _os.environ.get("SER_F16M_OUT_M", "0") == "1")
        return dict(qkv_mode=self.qkv_mode, x_mode=self.x_mode, qkv_out_mode=self.qkv_out_mode, gate_in_attn=self.gate_in_attn, out_m=False)

    def _check_last_state(self, last_state: Optional[int]) -> Optional[int]:
        if last_state is None:
            return None
        L = self.geo.num_layers
        last_state = int(last_state)
        if not 0 <= last_state <= L:
            raise IndexError("tuple index out of range")         # what hidden_states[N] raises in the reference
        return None if last_state == L else last_state

    def _state_done(self, i: int, last_state: Optional[int]) -> bool:
        """Hidden state ``i`` is complete; True = stop here.  ``last_state`` = N: the caller reads hidden_states[N] only (the reference's
        speech script keeps one state, preprocess_speech.py:67), so the layers that only feed later states are not launched.  Recording
        a command list marks where every state is complete instead (Tape.marks), and the replay stops there."""
        rec = self._rec
        if rec is None:
            return last_state == i
        rec.marks[i] = rec.n
        return False

    def _row_center(self, x: torch.Tensor, out_act: Act, stats: torch.Tensor, shift: torch.Tensor, rows: int, D: int):
        """hidden_states[0] -> centred operand copy + row partials + shift for encoder layer 0 (ser_row_center)."""
        groups = stats.shape[1]
        a = self._cmd("row_center")
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = x.data_ptr(), D, out_act.ptr, out_act.cols, out_act.plane_stride
        a.stats, a.shift, a.stat_groups, a.mode, a.rows, a.D = stats.data_ptr(), shift.data_ptr(), groups, self._lay_modes(0)["x_mode"], rows, D
        if out_act.scale is not None:
            a.out_scale, a.out_scale_ld = out_act.scale.data_ptr(), out_act.scale_ld
        a.range_flag = self._flag
        self._issue(_lib.OP_ROW_CENTER, a, "ser_row_center", rows=rows)

    def _attention(self, qkv: Act, frame_offs_dev, B, max_frames, out: Act, *, table=None, table_T=0, gate=None,
                   gru_const=None, key_lens=None, bias2d=None, gate_in=None, out_m=False):
        """``gate_in`` = (operand copy of the layer input, lnstat of the packed projection, folded weights, constants): the WavLM gate
        is computed inside the kernel (ser_attention_args.gate_x) instead of read from gate columns of ``qkv``."""
        D, H, dh = self.geo.hidden, self.geo.heads, self.geo.head_dim
        # column blocks of the packed projection: [q | k | v | gate] or, with the logit path on its own launch ("f16q"), [q | k | gate | v]
        q_col, k_col, v_col, gate_col = self._qkv_cols()
        amode = _lib.MODE_FP16Q if self.qk_mode is not None else self.attn_mode
        a = self._cmd("attention")
        a.qkv, a.ld, a.plane_stride = qkv.ptr, qkv.cols, qkv.plane_stride
        a.q_col, a.k_col, a.v_col, a.B = q_col, k_col, v_col, B
        a.frame_offs, a.table, a.gate = frame_offs_dev.data_ptr(), _ptr(table), _ptr(gate)
        a.max_frames, a.table_T = max_frames, table_T
        a.out, a.ldo, a.out_plane_stride = out.ptr, out.cols, out.plane_stride
        a.H, a.dh, a.scale, a.mode, a.gate_col = H, dh, -1.0, amode, gate_col       # q is pre-scaled
        if out_m:                                                                   # context rows as SER_MODE_FP16M operands (ABI 14)
            a.out_mode, a.out_scale, a.out_scale_ld = _lib.MODE_FP16M, out.scale.data_ptr(), out.scale_ld
        else:
            a.out_mode, a.out_scale, a.out_scale_ld = 0, None, 0
        a.gru_const, a.key_lens = _ptr(gru_const), _ptr(key_lens)
        a.bias2d, a.bias2d_ld = _ptr(bias2d), (0 if bias2d is None else bias2d.shape[-1])
        if gate_in is not None:
            xa, lnstat, gw, gcb = gate_in
            a.gate_x, a.gate_x_ld, a.gate_x_plane_stride, a.gate_x_planes = xa.ptr, xa.cols, xa.plane_stride, xa.planes
            a.gate_stat, a.gate_w, a.gate_cb = lnstat.data_ptr(), gw.data_ptr(), gcb.data_ptr()
            a.gate_w_plane_stride = gw.shape[1] * gw.shape[2]
        self._issue(_lib.OP_ATTENTION, a, "ser_attention", B=B, max_frames=max_frames, table_T=table_T)

    @staticmethod
    def _gate_in(pl, lay):
        return (pl["xa"], pl["gst"], lay["gate_w"], lay["gate_cb"]) if "gate_w" in lay else None

    def _gate_width(self) -> int:
        """the WavLM gate's two pre-activations per head as packed-projection columns, padded to a multiple of 8 (GEMM N)"""
        return ((2 * self.geo.heads + 7) // 8) * 8

    def _gate_pad(self) -> int:
        """extra columns of the stable-LN packed projection: the gate's, when some layer keeps the gate in the projection"""
        in_cols = any(not self._lay_modes(i)["gate_in_attn"] for i in range(self.geo.num_layers))
        return self._gate_width() if (self.geo.family == FAMILY_WAVLM and in_cols) else 0

    def _gate_cols(self, sd, a: str):
        """WavLM's gate as extra rows of a packed projection (HF modeling_wavlm.py:167-180): its two pre-activations per head are the sums
        of gru_rel_pos_linear's first and last four outputs over the head's dh input channels.  Returns (weight rows [_gate_width(), D],
        their bias, gru_rel_pos_const on the device); the padding rows are zero."""
        D, H, dh = self.geo.hidden, self.geo.heads, self.geo.head_dim
        w8, b8 = sd[a + ".gru_rel_pos_linear.weight"].float(), sd[a + ".gru_rel_pos_linear.bias"].float()
        wa, wb = w8[:4].sum(0), w8[4:].sum(0)
        wg = torch.zeros(self._gate_width(), D, device=w8.device)
        for h in range(H):
            wg[2 * h, h * dh:(h + 1) * dh] = wa
            wg[2 * h + 1, h * dh:(h + 1) * dh] = wb
        bg = torch.zeros(self._gate_width(), device=w8.device)
        bg[:2 * H] = torch.stack([b8[:4].sum(), b8[4:].sum()]).repeat(H)
        return wg, bg, self._dev_f32(sd[a + ".gru_rel_pos_const"].reshape(-1))

    def _qkv_cols(self):
        """(q, k, v, gate) first columns inside the packed projection output"""
        D = self.geo.hidden
        if self.qk_mode is None:
            return 0, D, 2 * D, 3 * D
        return 0, D, 2 * D + self._gate_pad(), 2 * D

    def _qkv_gemm(self, pl, lay, M: int, first: bool, gx: int, ln_mean) -> None:
        """packed Q K V (+ gate) projection with LayerNorm 1 deferred into it; q leaves multiplied by dh^-0.5 * log2(e).
        "f16q": two launches over the same operand copy -- [q | k | gate] as the 3-product FP16X GEMM on both planes of x,
        [v] as a single-product FP16 GEMM on its hi plane."""
        geo = self.geo
        D = geo.hidden
        stats = pl["px0"] if first else pl["px"]
        scale = geo.head_dim ** -0.5 * 1.4426950408889634
        lnstat = pl["gst"] if "gate_w" in lay else None     # (relative mean, rstd) per row for the attention kernel's in-kernel gate
        if self.qk_mode is None:
            self._gemm(pl["xa"], lay["qkv"], M, ln_stats=stats, ln_groups=gx, out_act=pl["qkv"], col_scale=scale,
                       col_scale_end=D, ln_mean=ln_mean, mode=lay["qkv_mode"], out_mode=lay["qkv_out_mode"], lnstat_out=lnstat)
            return
        self._gemm(pl["xa"], lay["qk"], M, ln_stats=stats, ln_groups=gx, out_act=pl["qkv"], col_scale=scale,
                   col_scale_end=D, ln_mean=ln_mean, mode=self.qk_mode, lnstat_out=lnstat)
        self._gemm(pl["xa"], lay["v"], M, ln_stats=stats, ln_groups=gx, out_act=pl["qkv"], out_col=self._qkv_cols()[2])

    def _attention_block(self, pl, lay, first: bool, gx: int, B: int, max_frames: int, residual: torch.Tensor, out_f32: torch.Tensor,
                         shifted: bool = True) -> None:
        """One stable-LN layer's attention block: packed QKV(+gate) projection -> attention -> output projection (+ ``residual`` ->
        ``out_f32``, operand copy ``ha``).  ``gx``: partial-sum groups of the layer input's producer; ``shifted``: the shifted operand
        copies (see _run_layers)."""
        M, D = pl["M"], self.geo.hidden
        gD = self._stat_groups(D)
        self._qkv_gemm(pl, lay, M, first, gx, (pl["sx"], pl["mx"]) if shifted else None)
        if self.geo.family == FAMILY_WAVLM:
            self._attention(pl["qkv"], pl["frame_offs"], B, max_frames, pl["ctx"], table=pl["table"],
                            table_T=pl["Tmax"], gru_const=lay["gate_c"], gate_in=self._gate_in(pl, lay), out_m=lay["out_m"])
        else:
            self._attention(pl["qkv"], pl["frame_offs"], B, max_frames, pl["ctx"], out_m=lay["out_m"])
        self._gemm(pl["ctx"], lay["out"], M, residual=residual, ldr=D, out_f32=out_f32, ldo_f32=D,
                   out_act=pl["ha"], stat_out=pl["ph"], stat_groups=gD, mode=_lib.MODE_FP16M if lay["out_m"] else self.attn_mode, out_mode=self.mode,
                   shift=(pl["mx"], pl["sh"], lay["out_bias_mean"]) if shifted else None)

    def _post_ln_tail(self, pl, lay, x: torch.Tensor, out_f32: torch.Tensor, out_act: Optional[Act]) -> None:
        """The rest of a post-LN layer once attention has written ``ctx``: [out GEMM + x] -> LN1 -> h (copy ha) -> [FC1 GEMM, GELU]
        -> [FC2 GEMM + h] -> LN2 -> ``out_f32`` and its operand copy ``out_act`` (None: no copy)."""
        M, D = pl["M"], self.geo.hidden
        self._gemm(pl["ctx"], lay["out"], M, residual=x, ldr=D, out_f32=pl["tmp"], ldo_f32=D)
        self._layernorm(pl["tmp"], D, lay["ln1"], M, D, out_f32=pl["h"], out_act=pl["ha"])
        self._gemm(pl["ha"], lay["fc1"], M, act=_lib.ACT_GELU, out_act=pl["ffn"])
        self._gemm(pl["ffn"], lay["fc2"], M, residual=pl["h"], ldr=D, out_f32=pl["tmp"], ldo_f32=D)
        self._layernorm(pl["tmp"], D, lay["ln2"], M, D, out_f32=out_f32, out_act=out_act)

    @staticmethod
    def _stat_groups(n_cols: int, groups: int = 1) -> int:
        """64-column partial-sum slots a GEMM output of `groups` x `n_cols` columns produces (made even)."""
        g = groups * ((n_cols + 63) // 64)
        return g + (g & 1)

    def _run_layers(self, pl, states, first_groups: int, B: int, max_frames: int, last_state: Optional[int] = None):
        """Pre-LN / stable-LN encoder layers with BOTH LayerNorms deferred into the consuming GEMMs:
        x -> [QKV(+gate) GEMM: LN1 folded] -> attention -> [out GEMM +x -> h] -> [FC1 GEMM: LN2 folded, GELU]
          -> [FC2 GEMM +h -> next x].  Producers emit the bf16 operand copy and the row partial sums, both SHIFTED by
        the row mean of their residual input: the consumer of x (QKV) reports x's absolute row mean (mx), the producer
        of h (out-proj) shifts by it and records the shift (sh), the consumer of h (FC1) reports mh, the producer of
        the next x (FC2) shifts by that (sx).  Offsets that live in the residual stream never reach the bf16 rounding or
        the one-pass variance.  states[0] is centred once by ser_row_center."""
        geo = self.geo
        M, D, L = pl["M"], geo.hidden, geo.num_layers
        gD = self._stat_groups(D)
        gx = first_groups
        if self._state_done(0, last_state):
            return
        self._row_center(states[0], pl["xa"], pl["px0"], pl["sx"], M, D)
        shifted = not _NO_SHIFT
        for i, lay in enumerate(self.layers):
            x = states[i]
            last = i + 1 == L
            nxt = pl["last"] if last else states[i + 1]
            if self.block_trace is not None:
                b0 = torch.cuda.Event(enable_timing=True)
                b0.record()
            self._attention_block(pl, lay, i == 0, gx, B, max_frames, x, pl["h"], shifted)
            if self.block_trace is not None:
                b1 = torch.cuda.Event(enable_timing=True)
                b1.record()
                self.block_trace.append((b0, b1, B))
            self._gemm(pl["ha"], lay["fc1"], M, ln_stats=pl["ph"], ln_groups=gD, act=_lib.ACT_GELU, out_act=pl["ffn"],
                       ln_mean=(pl["sh"], pl["mh"]) if shifted else None)
            if last:
                self._gemm(pl["ffn"], lay["fc2"], M, residual=pl["h"], ldr=D, out_f32=nxt, ldo_f32=D)
            else:
                self._gemm(pl["ffn"], lay["fc2"], M, residual=pl["h"], ldr=D, out_f32=nxt, ldo_f32=D,
                           out_act=pl["xa"], stat_out=pl["px"], stat_groups=gD, out_mode=self.layers[i + 1]["x_mode"],
                           shift=(pl["mh"], pl["sx"], lay["fc2_bias_mean"]) if shifted else None)
            gx = gD
            if not last and self._state_done(i + 1, last_state):
                return
        self._layernorm(pl["last"], D, self.enc_ln, M, D, out_f32=states[L])

    def _launch_or_replay(self, owner: dict, pl, packed_wave: torch.Tensor, last_state: Optional[int]) -> HiddenStates:
        """One forward of ``self._launches`` over ``owner`` (the slot's arena; Whisper: the plan), through ``_replay``"""
        flag = self._guard_word(pl)
        self._replay((owner,), pl.get("sizes", {}), lambda last: self._launches(pl, packed_wave, last), packed_wave.data_ptr(), last_state)
        return HiddenStates(pl["states"], pl["frame_offs_host"], None if last_state is None else last_state + 1, range_flag=flag,
                            frame_offs_dev=pl.get("frame_offs"))

    @_on_stream
    def attention_blocks_only(self, lengths: Sequence[int], slot: int) -> int:
        """Measurement aid (bench.py ``attention_block``): launch ONLY the attention sub-graph of every layer -- packed QKV(+gate)
        projection -> attention -> output projection -- over the buffers the slot's last forward left behind (same shapes,
        same kernels, stale but finite data), on the current stream.  Returns the number of layer calls."""
        pl = self._plan(lengths, slot)
        self._guard_word(pl)
        max_frames = pl.get("Tmax", self.geo.max_source_positions)
        gD = self._stat_groups(self.geo.hidden)
        for i, lay in enumerate(self.layers):
            self._attention_block(pl, lay, i == 0, pl["first_groups"] if i == 0 else gD, len(lengths), max_frames, pl["h"], pl["h"])
        return len(self.layers)

    def _layer_weights(self, sd, p: str, a: str, ln1: str, ln2: str, fc1: str, fc2: str, k_bias: bool, gate: bool, index: int = 0):
        """One encoder layer's GEMM operands; LN1 folds into the packed QKV (+gate) projection, LN2 into FC1."""
        D, H, dh = self.geo.hidden, self.geo.heads, self.geo.head_dim
        lm = self._lay_modes(index)
        wdev = sd[a + ".q_proj.weight"].device            # CPU state dict, or device views of the broadcast bucket (dist.py)
        kb = sd[a + ".k_proj.bias"] if k_bias else torch.zeros(D, device=wdev)
        ws = [sd[a + ".q_proj.weight"], sd[a + ".k_proj.weight"], sd[a + ".v_proj.weight"]]
        bs = [sd[a + ".q_proj.bias"], kb, sd[a + ".v_proj.bias"]]
        lay = dict(qkv_mode=lm["qkv_mode"], x_mode=lm["x_mode"], qkv_out_mode=lm["qkv_out_mode"], out_m=lm["out_m"])
        if gate and lm["gate_in_attn"]:
            # WavLM GRU gate (HF modeling_wavlm.py:167-180): its two pre-activations per head are linear in LN1(x) restricted to the
            # head's dh channels.  ser_attention evaluates them per query from the layer input's operand copy with the LayerNorm in
            # closed form (ser_attention_args.gate_x): pre_j = rstd (x . (gamma w_j) - mean sum(gamma w_j)) + (beta . w_j + b_j)
            from .weights import fold_wavlm_gate
            wg, t = fold_wavlm_gate(sd[a + ".gru_rel_pos_linear.weight"], sd[a + ".gru_rel_pos_linear.bias"],
                                    sd[ln1 + ".weight"], sd[ln1 + ".bias"], H, dh)
            # operand planes [planes][H][2][dh] in the format the attention launch multiplies in (one MFMA chain per query block)
            gmode = self.qk_mode if self.qk_mode is not None else self.attn_mode
            glin = self._linear(wg.float(), None, mode=gmode, name=a + ".gru_rel_pos_linear.weight (folded gate)")
            cs = glin.w.double().sum(dim=(0, 2)).view(H, 2)                             # column sums of exactly the planes the MFMAs read
            lay["gate_w"] = glin.w
            lay["gate_cb"] = self._dev_f32(torch.cat([cs.to(t.device), t], 1).float())
            lay["gate_c"] = self._dev_f32(sd[a + ".gru_rel_pos_const"].reshape(-1))
            gate = False                                                                # no gate columns in the packed projection
        if gate:
            # (SER_GATE_IN_ATTN=0, FP16M projections) the two pre-activations per head as extra output columns of the packed projection
            wg, bg, lay["gate_c"] = self._gate_cols(sd, a)
            ws.append(wg)
            bs.append(bg)
        if self.qk_mode is None:
            lay["qkv"] = self._linear_ln(torch.cat(ws, 0), torch.cat(bs, 0), sd[ln1 + ".weight"], sd[ln1 + ".bias"], mode=lm["qkv_mode"],
                                         name=a + ".{q,k,v}_proj.weight")
        else:
            # logit path [q | k | gate] on fp16 hi + lo planes (3 products), [v] on one fp16 plane
            lay["qk"] = self._linear_ln(torch.cat(ws[:2] + ws[3:], 0), torch.cat(bs[:2] + bs[3:], 0), sd[ln1 + ".weight"],
                                        sd[ln1 + ".bias"], mode=self.qk_mode, name=a + ".{q,k}_proj.weight")
            lay["v"] = self._linear_ln(ws[2], bs[2], sd[ln1 + ".weight"], sd[ln1 + ".bias"], name=a + ".v_proj.weight")
        lay["out"] = self._linear(sd[a + ".out_proj.weight"], sd[a + ".out_proj.bias"], mode=_lib.MODE_FP16M if lm["out_m"] else self.attn_mode,
                                  name=a + ".out_proj.weight")
        lay["fc1"] = self._linear_ln(sd[fc1 + ".weight"], sd[fc1 + ".bias"], sd[ln2 + ".weight"], sd[ln2 + ".bias"], name=fc1 + ".weight")
        lay["fc2"] = self._linear(sd[fc2 + ".weight"], sd[fc2 + ".bias"], name=fc2 + ".weight")
        # load-time part of the operand shift: a uniform offset in a bias moves the row mean by exactly its mean
        lay["out_bias_mean"] = float(sd[a + ".out_proj.bias"].double().mean())
        lay["fc2_bias_mean"] = float(sd[fc2 + ".bias"].double().mean())
        return lay

    def _post_ln_layer_weights(self, sd, q: str, k: str, v: str, out: str, ln1: str, fc1: str, fc2: str, ln2: str, gate=None) -> dict:
        """One post-LN layer (HF BERT / RoBERTa / DeBERTa, WavLMEncoderLayer / Wav2Vec2EncoderLayer) from the checkpoint key prefixes of
        its tensors: plain GEMM operands, the two LayerNorms run as ser_layernorm between them (the norm of a 768-wide row spans several
        GEMM tiles).  ``gate``: _gate_cols' WavLM gate, extra columns of the packed projection -- its pre-activations are linear in the
        attention's input, which here is the layer input itself."""
        def linear(p: str) -> Linear:
            return self._linear(sd[p + ".weight"], sd[p + ".bias"], name=p + ".weight")

        ws, bs = [sd[p + ".weight"] for p in (q, k, v)], [sd[p + ".bias"] for p in (q, k, v)]
        lay = {}
        if gate is not None:
            ws.append(gate[0])
            bs.append(gate[1])
            lay["gate_c"] = gate[2]
        lay["qkv"] = self._linear(torch.cat(ws, 0), torch.cat(bs, 0), name=" + ".join(p + ".weight" for p in (q, k, v)))
        lay["out"] = linear(out)
        lay["ln1"] = self._ln_pair(sd, ln1)
        lay["fc1"] = linear(fc1)
        lay["fc2"] = linear(fc2)
        lay["ln2"] = self._ln_pair(sd, ln2)
        return lay

    def _post_ln_buffers(self, pl, M: int, nqkv: int) -> None:
        """Activation set of M rows of post-LN layers (_post_ln_tail), packed projection ``nqkv`` columns wide: operand copies of the
        layer input (xa), of LN1's output (ha), of the context rows, of the projection and of FC1's output; LN1's / LN2's fp32 input
        (tmp) and LN1's output (h)."""
        D, dev = self.geo.hidden, self.device
        pl["xa"], pl["ha"], pl["ctx"] = self._new_act(M, D), self._new_act(M, D), self._new_act(M, D)
        pl["qkv"], pl["ffn"] = self._new_act(M, nqkv), self._new_act(M, self.geo.ffn)
        pl["tmp"] = torch.empty((M, D), dtype=torch.float32, device=dev)
        pl["h"] = torch.empty((M, D), dtype=torch.float32, device=dev)
        if self.fp16_planes:
            pl["range_flag"] = torch.zeros(1, dtype=torch.int32, device=dev)   # the slot's fp16 range-guard word (HiddenStates.range_flag)

    def _layer_buffers(self, pl, M: int, first_groups: int):
        geo, dev = self.geo, self.device
        D, Fd = geo.hidden, geo.ffn
        nqkv = 3 * D + self._gate_pad()
        gD = self._stat_groups(D)
        # (an FP16M buffer serves FP16X layers too: same two fp16-sized planes, the block-scale words are simply not touched)
        x_modes = {self._lay_modes(i)["x_mode"] for i in range(geo.num_layers)}
        pl["xa"] = self._new_act(M, D, mode=_lib.MODE_FP16M if _lib.MODE_FP16M in x_modes else self.x_mode)
        pl["ha"] = self._new_act(M, D)
        if self.fp16_planes:
            pl["range_flag"] = torch.zeros(1, dtype=torch.int32, device=dev)   # the slot's fp16 range-guard word (HiddenStates.range_flag)
        # row partial sums (sum, sum^2 per 64-column group).  One buffer per producer layout: a padding
        # slot (odd group count) is never written and must stay zero.
        pl["px0"] = torch.zeros((M, first_groups, 2), dtype=torch.float32, device=dev)   # states[0] (ser_row_center)
        pl["sx"] = torch.zeros(M, dtype=torch.float32, device=dev)       # row shift of the xa copy / px partials
        pl["sh"] = torch.zeros(M, dtype=torch.float32, device=dev)       # row shift of the ha copy / ph partials
        pl["mx"] = torch.zeros(M, dtype=torch.float32, device=dev)       # absolute row mean of x (written by the QKV GEMM)
        pl["mh"] = torch.zeros(M, dtype=torch.float32, device=dev)       # absolute row mean of h (written by the FC1 GEMM)
        pl["gst"] = torch.zeros((M, 2), dtype=torch.float32, device=dev)  # (relative mean, rstd) of x's rows (packed projection -> attention's gate)
        pl["px"] = torch.zeros((M, gD, 2), dtype=torch.float32, device=dev)              # FC2 outputs
        pl["ph"] = torch.zeros((M, gD, 2), dtype=torch.float32, device=dev)              # out-proj outputs
        pl["qkv"] = self._new_act(M, nqkv, mode=self._lay_modes(geo.num_layers - 1)["qkv_out_mode"])   # "f16q": q, k, gate columns carry a lo plane, v's stays unused
        any_out_m = any(self._lay_modes(i)["out_m"] for i in range(geo.num_layers))
        pl["ctx"] = self._new_act(M, D, mode=_lib.MODE_FP16M if any_out_m else self.attn_mode)   # (an FP16M buffer serves the FP16X layers too)
        pl["h"] = torch.empty((M, D), dtype=torch.float32, device=dev)
        pl["ffn"] = self._new_act(M, Fd)
        pl["last"] = torch.empty((M, D), dtype=torch.float32, device=dev)

    def capture(self, packed_wave: torch.Tensor, lengths: Sequence[int]):
        """Record one forward over a fixed batch shape into a hipGraph (via torch's CUDAGraph
        plumbing).  A forward is ~230 short launches; replaying the graph removes the host-side
        launch gaps that otherwise cost ~25 % of a step.  Returns (graph, hidden_states): the
        states tensor is overwritten in place by every ``graph.replay()``."""
        self._plan(lengths)                                  # buffers + offset tables allocated before capture
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.forward(packed_wave, lengths)               # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hs = self.forward(packed_wave, lengths)
        return graph, hs

    def capture_concurrent(self, micro_batches):
        """Record the forwards of several independent micro-batches as PARALLEL branches of one
        hipGraph (one HIP stream each).  Every GEMM of this path spends a third of its time in a
        memory-bound prologue/epilogue during which the matrix cores idle; with two utterance
        groups in flight the tail of one group's kernel overlaps the main loop of the other's.
        ``micro_batches`` = [(packed_wave, lengths), ...]; returns (graph, [HiddenStates, ...])."""
        for slot, (wave, lengths) in enumerate(micro_batches):
            self._plan(lengths, slot)
        warm = torch.cuda.Stream(device=self.device)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            for slot, (wave, lengths) in enumerate(micro_batches):
                self.forward(wave, lengths, slot=slot)
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        sides = [torch.cuda.Stream(device=self.device) for _ in micro_batches[1:]]
        graph = torch.cuda.CUDAGraph()
        outs = [None] * len(micro_batches)
        with torch.cuda.graph(graph):
            main = torch.cuda.current_stream()
            for st in sides:
                st.wait_stream(main)                                   # fork
            for slot, st in enumerate(sides, start=1):
                with torch.cuda.stream(st):
                    outs[slot] = self.forward(*micro_batches[slot], slot=slot)
            outs[0] = self.forward(*micro_batches[0], slot=0)
            for st in sides:
                main.wait_stream(st)                                   # join
        return graph, outs

    def _ln_pair(self, sd, prefix):
        return (self._dev_f32(sd[prefix + ".weight"]), self._dev_f32(sd[prefix + ".bias"]))


def _fold_weight_norm(sd) -> torch.Tensor:
    """w = g * v / ||v||_(dims 0,1) per tap (HF modeling_wavlm.py:48-75), at load time."""
    base = "encoder.pos_conv_embed.conv."
    if base + "parametrizations.weight.original0" in sd:
        g, v = sd[base + "parametrizations.weight.original0"], sd[base + "parametrizations.weight.original1"]
    elif base + "weight_g" in sd:
        g, v = sd[base + "weight_g"], sd[base + "weight_v"]
    else:
        return sd[base + "weight"].float()
    g, v = g.float(), v.float()
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


def _halo_layout(tab: TableBlob, offs, offs_dev, half: int, width: int, rowmap, rowoffs, halo: Act, taps=None):
    """The zero-halo'd copy of a ragged batch: [half zero rows][utt 0][half zero rows][utt 1] ... [half zero rows]; row t of utterance b
    sits at ``starts[b] + t``, starts[b] = half (b + 1) + offs[b], and a convolution's taps begin ``taps[j]`` (default: half) rows
    earlier.  Puts the O(B) base rows into ``tab`` and returns (starts, the function that builds the O(rows) tables once ``tab`` is
    sent): the row map into ``rowmap``, the tap offsets (16-byte units of ``width``-column rows) into ``rowoffs[j]``, and zeroes ``halo``
    when an earlier plan left rows where this one's halo lies."""
    B, M = len(offs) - 1, int(offs[-1])
    starts = half * np.arange(1, B + 1, dtype=np.int64) + np.asarray(offs[:B], dtype=np.int64)
    bases = [tab.put64(starts)] + [tab.put64(starts - t) for t in (taps or (half,))]

    def index(st: int, rezero: bool) -> None:
        check(lib.ser_ragged_index(offs_dev.data_ptr(), bases[0].data_ptr(), B, 1, 1, 1, rowmap.data_ptr(), M, st), "ser_ragged_index")
        for base, out in zip(bases[1:], rowoffs):
            check(lib.ser_ragged_index(offs_dev.data_ptr(), base.data_ptr(), B, 1, width, 8, out.data_ptr(), M, st), "ser_ragged_index")
        if rezero:
            halo.t.zero_()
    return starts, index


class _WaveIO:
    """Waveform I/O of the encoders that take raw samples: ``upload`` / ``upload_resampled`` (host -> packed device buffer) and ``download``.
    A mixin in front of a ``_LaunchHost`` (it reads ``self.device``)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._pin_in: Dict[int, Pinned] = {}                # slot -> pinned staging buffer of ``upload``
        self._rs_tabs: Dict[int, TableBlob] = {}            # slot -> ser_resample_v's O(B) tables
        self._rs_banks = dict(buf=None, used=0, offs={}, retired=[])      # the polyphase banks met so far, one float64 device buffer

    def upload(self, waves: Sequence[np.ndarray], slot: int = 0) -> torch.Tensor:
        """Pack raw fp32 waveforms into slot ``slot``'s (reused, grow-only) pinned host buffer and copy H2D.
        The copy is enqueued on the current stream; the staging buffer is reused only after an event
        recorded behind its previous copy has completed."""
        total = int(sum(len(w) for w in waves))
        if total and all(isinstance(w, np.ndarray) and w.dtype == np.float32 and w.flags.c_contiguous for w in waves):
            srcs = [torch.from_numpy(w) for w in waves]
            if all(t.is_pinned() for t in srcs):
                # every utterance already sits in page-locked memory (driver: frontend.load_wav_16k(pinned=True)): one async copy each,
                # no packing pass here; torch's host allocator keeps a block from being re-issued until the copy from it has run
                dev = torch.empty(total, dtype=torch.float32, device=self.device)
                o = 0
                for t in srcs:
                    dev[o:o + t.numel()].copy_(t, non_blocking=True)
                    o += t.numel()
                return dev
        pin = self._pin_in.get(slot)
        if pin is None or pin.host.numel() < total:
            pin = self._pin_in[slot] = Pinned(max(total, 1 << 20), torch.float32)
        pin.wait()
        host = pin.host[:total]
        view = host.numpy()
        o = 0
        for w in waves:
            n = len(w)
            view[o:o + n] = w
            o += n
        dev = host.to(self.device, non_blocking=True)
        pin.sent()
        return dev

    def _resample_bank(self, up: int, down: int):
        """(element offset, half) of the (up, down) polyphase bank inside this encoder's float64 bank buffer on the device; a ratio met
        for the first time is appended (one blocking copy per ratio and encoder).  Appending never moves what launches in flight read: a
        buffer that runs out of room is succeeded by a larger one and kept alive beside it."""
        from .frontend import polyphase_bank
        rs = self._rs_banks
        hit = rs["offs"].get((up, down))
        if hit is not None:
            return hit
        h, half = polyphase_bank(up, down)
        if rs["buf"] is None or rs["used"] + len(h) > rs["buf"].numel():
            grown = torch.empty(max(1 << 16, 2 * (rs["used"] + len(h))), dtype=torch.float64, device=self.device)
            if rs["buf"] is not None:
                grown[: rs["used"]].copy_(rs["buf"][: rs["used"]])
                rs["retired"].append(rs["buf"])
            rs["buf"] = grown
        off = rs["used"]
        rs["buf"][off: off + len(h)].copy_(torch.from_numpy(h.copy()))      # the cached bank is read-only
        torch.cuda.current_stream().synchronize()           # every slot's stream may read the bank from now on
        rs["used"] = off + len(h)
        rs["offs"][(up, down)] = (off, half)
        return off, half

    def upload_resampled(self, waves: Sequence[np.ndarray], rates: Sequence[int], slot: int = 0):
        """``upload`` for utterances at their files' own sample rates: stages the raw samples like ``upload`` does, and enqueues ONE
        ``ser_resample_v`` launch on the current stream that brings the ragged, mixed-rate batch to 16 kHz (Kaiser beta 14 polyphase
        FIR, the ``--resample`` filter of frontend.load_wav_16k; parity with librosa's soxr_hq unpinned).  Returns (packed 16 kHz
        device buffer, lengths) for ``forward``.  A batch that is all 16 kHz goes through plain ``upload``."""
        from .frontend import TARGET_SR, resample_ratio
        rates = [int(r) for r in rates]
        if len(rates) != len(waves):
            raise ValueError("one sample rate per utterance")
        if all(r == TARGET_SR for r in rates):
            return self.upload(waves, slot), [len(w) for w in waves]
        B = len(waves)
        ratios = [resample_ratio(r) for r in rates]
        n_in = [len(w) for w in waves]
        n_out = [(n * u + d - 1) // d for n, (u, d) in zip(n_in, ratios)]
        banks = [(0, 0) if u == d == 1 else self._resample_bank(u, d) for u, d in ratios]
        raw = self.upload(waves, slot)
        # ---- O(B) tables -> this slot's blob, replaced by a larger one when B outgrows it
        tab = self._rs_tabs.get(slot)
        if tab is None or tab.layout.region < B + 2:
            tab = self._rs_tabs[slot] = TableBlob(max(B, 16), 6, self.device)
        tab.begin()
        tabs = [tab.put64(np.concatenate([[0], np.cumsum(n)])) for n in (n_in, n_out)] + [tab.put64([o for o, _ in banks])]
        tabs += [tab.put32(v) for v in ([u for u, _ in ratios], [d for _, d in ratios], [hf for _, hf in banks])]
        tab.send()
        out = torch.empty(int(sum(n_out)), dtype=torch.float32, device=self.device)
        a = _lib.ResampleArgs()
        a.wav = raw.data_ptr()
        a.in_offs, a.out_offs, a.bank_off, a.up, a.down, a.half = (t.data_ptr() for t in tabs)
        a.bank, a.out = self._rs_banks["buf"].data_ptr(), out.data_ptr()
        a.total_in, a.total_out, a.max_out, a.B = int(sum(n_in)), int(sum(n_out)), int(max(n_out)), B
        check(lib.ser_resample_v(C.byref(a), _stream()), "ser_resample_v")
        return out, n_out

    def download(self, t: torch.Tensor) -> torch.Tensor:
        """Device fp32 tensor -> fresh pinned host tensor (async D2H + one synchronisation)."""
        host = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return host


class SpeechEncoder(_WaveIO, _EncoderBase):
    """WavLM / wav2vec2 / HuBERT on libserhip: the *-large / xlarge / XLS-R form (layer-norm conv stack, stable-LayerNorm encoder) and
    the *-base form (GroupNorm-over-time conv layer 0, post-LayerNorm encoder; ``geo.stable_layer_norm`` False).  data2vec-audio: the
    layer-norm conv stack with a post-LayerNorm encoder, and a stack of LayerNorm'd positional convs (``geo.pos_conv_norm == "layer"``).
    ``normalize``: the feature extractor's ``do_normalize`` (zero-mean / unit-variance input per utterance)."""

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "bf16", normalize: bool = True):
        super().__init__(geo, device, mode, post_ln=not geo.stable_layer_norm)
        if geo.family == FAMILY_WHISPER:
            raise ValueError("use WhisperEncoder for the whisper family")
        self.normalize = bool(normalize)
        self.gn_stem = geo.feat_extract_norm == "group"
        if (geo.family == FAMILY_DATA2VEC_AUDIO) != (geo.pos_conv_norm == "layer"):
            raise NotImplementedError("the LayerNorm'd positional conv stack is data2vec-audio's, and data2vec-audio has only that one")
        if geo.family == FAMILY_DATA2VEC_AUDIO:
            if self.gn_stem or not self.post_ln:
                raise NotImplementedError("data2vec-audio: the layer-norm conv stem with a post-LN encoder is the only form")
        elif self.post_ln != self.gn_stem:
            raise NotImplementedError("GroupNorm stems come with post-LN encoders and layer-norm stems with stable-LN ones")
        if not geo.feat_proj_layer_norm:
            raise NotImplementedError("feat_proj_layer_norm=False checkpoints are not supported")
        sd = state_dict
        D = geo.hidden
        self._init_stem(sd)
        # positional conv: per group [Cg out][tap][Cg in padded to a multiple of 64]
        G, k = geo.pos_conv_groups, geo.pos_conv_kernel
        Cg = D // G
        self.pos_cg, self.pos_kc = Cg, ((Cg + 63) // 64) * 64

        def pos_weight(w: torch.Tensor) -> torch.Tensor:                  # [D, Cg, k] -> [G * Cg, k * pos_kc]
            wp = torch.zeros((G, Cg, k, self.pos_kc), dtype=torch.float32)
            wp[:, :, :, :Cg] = w.float().view(G, Cg, Cg, k).permute(0, 1, 3, 2)
            return wp.reshape(G * Cg, k * self.pos_kc)
        # The positional conv runs in the LAYER format when its dot products are short enough: in "f16" mode it then costs 3x
        # less than on the fp32x stem and, unlike the conv stack and the projection, moves the error by nothing measurable
        # (WavLM-large, K = 128 taps x 64 channels: 6.8e-4 either way; HuBERT-xlarge, 128 x 80: 8.0e-4 either way).  XLS-R-2B's
        # 128 x 120 = 15 360-long sums do feel fp16 operands (7.0e-4 -> 8.3e-4 at full geometry), so they stay on the stem format.
        # "f16q" / "f16a" keep it on the stem format always: an error in hidden_states[0] enters layer 0's logits, and these modes
        # exist for attention maps sharp enough to amplify it (LoRA stress fixture: 1.4e-3 -> see DESIGN.md section 4)
        self.pos_in_stem = (self.mode_name == "f16" and Cg * k > 128 * 80) or self.mode_name in ("f16q", "f16a", "f16m", "f16mf")
        if geo.pos_conv_norm == "layer":
            # data2vec-audio: pos_conv_layers grouped convs, each one GEMM over the halo'd copy followed by ser_pos_ln_v
            self.pos_stack = [self._linear(pos_weight(sd[f"encoder.pos_conv_embed.layers.{j}.conv.weight"]),
                                           sd[f"encoder.pos_conv_embed.layers.{j}.conv.bias"], stem=self.pos_in_stem,
                                           name=f"encoder.pos_conv_embed.layers.{j}.conv.weight") for j in range(geo.pos_conv_layers)]
        else:
            self.pos = self._linear(pos_weight(_fold_weight_norm(sd)), sd["encoder.pos_conv_embed.conv.bias"], stem=self.pos_in_stem,
                                    name="encoder.pos_conv_embed.conv.weight (weight-norm folded)")
        self.enc_ln = self._ln_pair(sd, "encoder.layer_norm")
        self.layers = []
        for i in range(geo.num_layers):
            p = f"encoder.layers.{i}"
            if self.post_ln:
                a = p + ".attention"
                self.layers.append(self._post_ln_layer_weights(
                    sd, a + ".q_proj", a + ".k_proj", a + ".v_proj", a + ".out_proj", p + ".layer_norm",
                    p + ".feed_forward.intermediate_dense", p + ".feed_forward.output_dense", p + ".final_layer_norm",
                    gate=self._gate_cols(sd, a) if geo.family == FAMILY_WAVLM else None))
                continue
            self.layers.append(self._layer_weights(
                sd, p, p + ".attention", p + ".layer_norm", p + ".final_layer_norm",
                p + ".feed_forward.intermediate_dense", p + ".feed_forward.output_dense",
                k_bias=True, gate=(geo.family == FAMILY_WAVLM), index=i))
        if geo.family == FAMILY_WAVLM:
            self.rel_embed = self._dev_f32(sd["encoder.layers.0.attention.rel_attn_embed.weight"])
        self._arenas = SlotArenas(self._build_arena)          # per slot; ar["plan"]: the plan currently laid out in it

    def _init_stem(self, sd) -> None:
        """The convolutional waveform encoder and the feature projection (HF *FeatureEncoder / *FeatureProjection): weights of the wav2vec2-style
        stem every family of this class -- and the conformer encoders behind it -- shares."""
        geo = self.geo
        self.gn_stem = geo.feat_extract_norm == "group"
        if not geo.feat_proj_layer_norm:
            raise NotImplementedError("feat_proj_layer_norm=False checkpoints are not supported")
        C0 = geo.conv_dim[0]
        if any(c != C0 for c in geo.conv_dim):
            raise NotImplementedError("conv_dim must be uniform")
        # conv stack
        p0 = "feature_extractor.conv_layers.0"
        self.conv0_w = self._dev_f32(sd[p0 + ".conv.weight"].reshape(C0, geo.conv_kernel[0]))
        self.conv0_b = self._dev_f32(sd[p0 + ".conv.bias"]) if geo.conv_bias else None
        # matrix-core form of conv layer 0: taps zero-padded to K = 64 (frames come from ser_wave_frames)
        if geo.conv_kernel[0] > 64:
            raise NotImplementedError("conv layer 0 kernel wider than 64 taps")
        w0 = torch.zeros((C0, 64), dtype=torch.float32)
        w0[:, : geo.conv_kernel[0]] = sd[p0 + ".conv.weight"].reshape(C0, geo.conv_kernel[0]).float()
        self.conv0 = self._linear(w0, sd[p0 + ".conv.bias"] if geo.conv_bias else None, stem=True, name=p0 + ".conv.weight")
        if self.gn_stem:        # GroupNorm(C, C) of conv layer 0 (its affine); layers 1..6 have no norm
            self.gn0 = self._ln_pair(sd, p0 + ".layer_norm")
            self.conv_ln = [None] * len(geo.conv_dim)
        else:
            self.conv_ln = [self._ln_pair(sd, f"feature_extractor.conv_layers.{i}.layer_norm") for i in range(len(geo.conv_dim))]
        self.convs: List[Linear] = []
        for i in range(1, len(geo.conv_dim)):
            p = f"feature_extractor.conv_layers.{i}.conv"
            w = sd[p + ".weight"].float()                                  # [Cout, Cin, k]
            w2 = w.permute(0, 2, 1).reshape(w.shape[0], -1)                # K index = tap*Cin + c
            self.convs.append(self._linear(w2, sd[p + ".bias"] if geo.conv_bias else None, stem=True, name=p + ".weight"))
        self.proj_ln = self._ln_pair(sd, "feature_projection.layer_norm")
        self.proj = self._linear(sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"], stem=True,
                                 name="feature_projection.projection.weight")

    # ------------------------------------------------------------------ per-slot arenas + plans
    def _build_arena(self, cap: Dict[str, int]) -> dict:
        """Buffer set of one slot (arena.SlotArenas): a stream of ragged batches re-uses the same HBM instead of allocating ~25 tensors
        per batch.  ``cap``: rows after conv 0 / conv 1, frames M, halo'd rows, utterances B, longest utterance Tmax."""
        geo, dev = self.geo, self.device
        C0, D = geo.conv_dim[0], geo.hidden
        nl = len(geo.conv_dim)
        ar = {}
        self._stem_arena(ar, cap)
        ar["halo_rowmap"] = torch.empty(cap["M"], dtype=torch.int32, device=dev)
        ar["pos_rowoff"] = torch.empty(cap["M"], dtype=torch.int32, device=dev)
        ar["proj_f32"] = torch.empty((cap["M"], D), dtype=torch.float32, device=dev)
        ar["halo_act"] = self._new_act(cap["halo"], D, zero=True, extra_rows=1, stem=self.pos_in_stem)
        ar["states"] = torch.empty((geo.num_layers + 1, cap["M"], D), dtype=torch.float32, device=dev)
        ar["first_groups"] = 2                               # ser_row_center writes one (sum, sum^2) slot + one zero slot
        if self.post_ln:
            self._post_ln_buffers(ar, cap["M"], 3 * D + (self._gate_width() if geo.family == FAMILY_WAVLM else 0))
        else:
            self._layer_buffers(ar, cap["M"], ar["first_groups"])
        if geo.family == FAMILY_WAVLM:
            ar["table"] = torch.empty(geo.heads * (2 * cap["Tmax"] - 1), dtype=torch.float32, device=dev)
        # the O(B) tables: sample_offs | offs[0..nl) (int32) | conv bases [1..nl) | halo base | pos base
        ar["tab"] = TableBlob(cap["B"], 1 + nl + (nl - 1) + 2, dev)
        return ar

    def _stem_arena(self, ar: dict, cap: Dict[str, int]) -> None:
        """the stem's buffers of one slot: ``cap`` rows after conv 0 / conv 1, frames M, utterances B"""
        geo, dev = self.geo, self.device
        C0, nl = geo.conv_dim[0], len(geo.conv_dim)
        ar["frames"] = self._new_act(cap["rows0"], 64, stem=True)
        ar["wave_work"] = torch.empty(lib.ser_workspace_bytes(_lib.WS_WAVE_FRAMES, cap["B"], 0, 0, 0, self.stem_mode),
                                      dtype=torch.uint8, device=dev)
        ar["conv_act"] = [self._new_act(cap["rows0"], C0, stem=True), self._new_act(cap["rows1"], C0, stem=True)]       # ping-pong
        ar["conv_rowoff"] = [torch.empty(cap["rows1"], dtype=torch.int32, device=dev) for _ in range(1, nl)]
        ar["feat_f32"] = torch.empty((cap["M"], C0), dtype=torch.float32, device=dev)
        ar["feat_act"] = self._new_act(cap["M"], C0, stem=True)
        if self.gn_stem:
            # the GroupNorm stem's per-(utterance, channel) affine + its workspace
            ar["gn_scale"] = torch.empty((cap["B"], C0), dtype=torch.float32, device=dev)
            ar["gn_shift"] = torch.empty((cap["B"], C0), dtype=torch.float32, device=dev)
            ar["gn_work"] = torch.empty(lib.ser_workspace_bytes(_lib.WS_GN_STATS, cap["B"], 0, 0, 0, self.stem_mode), dtype=torch.uint8, device=dev)

    def _stem_offsets(self, lengths: Sequence[int]):
        """per conv layer i the [B + 1] first rows of every utterance after it (int64); the last one's are the frame offsets"""
        chains = [self.geo.frame_chain(n) for n in lengths]
        if len(lengths) == 0 or min(c[-1] for c in chains) < 1:
            raise ValueError("utterance shorter than the conv stack's receptive field (400 samples)")
        return [np.concatenate([[0], np.cumsum([c[i] for c in chains])]).astype(np.int64) for i in range(len(self.geo.conv_dim))]

    def _stem_tables(self, pl: dict, tab: TableBlob, lengths: Sequence[int], offs):
        """the stem's O(B) tables into the blob (sample offsets, the per-layer offsets, the conv layers' base rows: 2 nl regions) and the
        sizes a recorded list patches; returns (device offsets per layer, base rows per conv layer 1..)"""
        B, nl = len(lengths), len(offs)
        pl["rows"] = [Sz(int(o[-1]), f"rows{i}") for i, o in enumerate(offs)]
        pl["sizes"] = {f"rows{i}": int(r) for i, r in enumerate(pl["rows"])}
        pl["sample_offs"] = tab.put64(np.concatenate([[0], np.cumsum(lengths)]))
        offs_dev = [tab.put32(o) for o in offs]             # offs[i][b] = first row of utterance b after conv layer i
        pl["frame_offs0"] = offs_dev[0]
        pl["frame_offs"] = offs_dev[-1]
        pl["frame_offs_host"] = [int(x) for x in offs[-1]]
        return offs_dev, [tab.put64(offs[i - 1][:B]) for i in range(1, nl)]

    def _stem_index(self, pl: dict, ar: dict, offs_dev, base_conv, st: int) -> None:
        """the conv layers' O(rows) row tables, on the device (after the blob was sent)"""
        geo = self.geo
        B, C0 = len(pl["lengths"]), geo.conv_dim[0]
        rowoffs = []
        for i in range(1, len(geo.conv_dim)):
            out = ar["conv_rowoff"][i - 1][: pl["rows"][i]]
            check(lib.ser_ragged_index(offs_dev[i].data_ptr(), base_conv[i - 1].data_ptr(), B, geo.conv_stride[i], C0, 8,
                                       out.data_ptr(), pl["rows"][i], st), "ser_ragged_index")
            rowoffs.append(out)
        pl["conv_rowoff"] = rowoffs

    def _plan(self, lengths: Sequence[int], slot: int = 0):
        """Row bookkeeping of one ragged batch in slot ``slot``'s arena.  Only O(B) integers are computed on the
        host and uploaded (one pinned blob, one async copy); the O(rows) row tables are built on the device by
        ``ser_ragged_index``.  A repeat of the previous lengths (benchmark, graph replay) re-uses the laid-out plan.
        The returned buffers -- including the hidden states -- stay valid until the next plan of the same slot."""
        lengths = tuple(int(n) for n in lengths)
        geo, dev = self.geo, self.device
        B = len(lengths)
        nl = len(geo.conv_dim)
        offs = self._stem_offsets(lengths)
        T = [int(t) for t in np.diff(offs[-1])]
        M, Tmax = int(offs[-1][-1]), max(T)
        half = geo.pos_conv_kernel // 2
        halo_rows = int(M + half * (B + 1))
        ar = self._arenas.fit(slot, rows0=int(offs[0][-1]), rows1=int(offs[1][-1]) if nl > 1 else 1, M=M, halo=halo_rows, B=B, Tmax=Tmax)
        if ar["plan"] is not None and ar["plan"]["lengths"] == lengths:
            return ar["plan"]
        st = _stream()
        C0, D = geo.conv_dim[0], geo.hidden
        tab = ar["tab"].begin()
        pl = dict(ar)                                       # arena buffers + this batch's views / numbers
        offs_dev, base_conv = self._stem_tables(pl, tab, lengths, offs)
        pl["sizes"].update(M=M, B=B, Tmax=Tmax)
        pl.update(B=Sz(B, "B"), lengths=lengths, T=T, M=Sz(M, "M"), Tmax=Sz(Tmax, "Tmax"), halo_rows=halo_rows)
        # halo'd layout of the positional-conv input: [64 zero rows][utt 0][64 zero rows][utt 1] ... [64 zero rows]
        _, halo_index = _halo_layout(tab, offs[-1], offs_dev[-1], half, D, ar["halo_rowmap"], [ar["pos_rowoff"]], ar["halo_act"])
        tab.send()
        # ---- O(rows) tables on the device
        self._stem_index(pl, ar, offs_dev, base_conv, st)
        halo_index(st, ar["plan"] is not None)
        pl["states"] = ar["states"][:, :M]
        if geo.family == FAMILY_WAVLM:
            pl["table"] = ar["table"][: geo.heads * (2 * Tmax - 1)].view(geo.heads, 2 * Tmax - 1)
            if ar.get("table_T") != Tmax:
                check(lib.ser_wavlm_bias_table(self.rel_embed.data_ptr(), pl["table"].data_ptr(), Tmax, geo.heads,
                                               geo.num_buckets, geo.max_bucket_distance, st), "ser_wavlm_bias_table")
                ar["table_T"] = Tmax
        ar["plan"] = pl
        return pl

    # ------------------------------------------------------------------ forward
    @_on_stream
    def forward(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0,
                last_state: Optional[int] = None) -> HiddenStates:
        """packed raw samples [sum(lengths)] fp32 on the device -> L+1 hidden states (``last_state`` = N: only states 0..N,
        the launches that feed later states are skipped)."""
        pl = self._plan(lengths, slot)
        return self._launch_or_replay(self._arenas[slot], pl, packed_wave, self._check_last_state(last_state))

    def _launches(self, pl, packed_wave: torch.Tensor, last_state: Optional[int] = None) -> None:
        geo = self.geo
        B, M, D = pl["B"], pl["M"], geo.hidden
        self._conv_stack(pl, packed_wave)
        # a9 (its Linear): the feature projection; also scatter into the zero-halo'd pos-conv input
        self._gemm(pl["feat_act"], self.proj, M, out_f32=pl["proj_f32"], ldo_f32=D,
                   out_act=pl["halo_act"], out_rowmap=pl["halo_rowmap"], stem=True,
                   out_mode=self.stem_mode if self.pos_in_stem else self.mode)
        states = pl["states"]
        G, Cg, kc = geo.pos_conv_groups, self.pos_cg, self.pos_kc
        if geo.pos_conv_norm == "layer":
            # data2vec-audio: hidden_states[0] = encoder.layer_norm(proj + stack(proj)) (HF Data2VecAudioEncoder.forward), then the layers
            self._pos_stack(pl, states)
            self._run_post_ln_layers(pl, states, B, pl["Tmax"], last_state)
            return
        # a10: grouped positional conv + GELU + residual -> hidden_states[0]
        self._gemm(pl["halo_act"], self.pos, M, a_rowoff=pl["pos_rowoff"], kc=kc, ldj=D, groups=G,
                   a_group_stride=Cg, w_group_stride=Cg * geo.pos_conv_kernel * kc, c_group_stride=Cg,
                   N=Cg, K=geo.pos_conv_kernel * kc, act=_lib.ACT_GELU, residual=pl["proj_f32"], ldr=D,
                   out_f32=pl["tmp"] if self.post_ln else states[0], ldo_f32=D, k_algo=geo.pos_conv_kernel * Cg, stem=self.pos_in_stem)
        if self.post_ln:
            # post-LN encoder: hidden_states[0] = encoder.layer_norm(proj + posconv(proj)) (HF WavLMEncoder), then the layers
            self._layernorm(pl["tmp"], D, self.enc_ln, M, D, out_f32=states[0], out_act=pl["xa"])
            self._run_post_ln_layers(pl, states, B, pl["Tmax"], last_state)
            return
        # a11/a12: stable-LayerNorm encoder layers (LayerNorms deferred into the GEMMs)
        self._run_layers(pl, states, pl["first_groups"], B, pl["Tmax"], last_state)

    def _conv_stack(self, pl, packed_wave: torch.Tensor) -> None:
        """packed samples -> the feature projection's LayerNorm'd operand rows ``feat_act`` [M, C0]"""
        geo = self.geo
        M, C0 = pl["M"], geo.conv_dim[0]
        # a6 + a7 (layer 0): zero-mean / unit-variance per utterance fused with framing, then
        # Conv1d(1,C,10,5)+LayerNorm+GELU on the matrix cores (K padded to 64, LayerNorm epilogue)
        self._wave_frames(pl, packed_wave)
        a_in = pl["conv_act"][0]
        if self.gn_stem:
            self._groupnorm_stem(pl, packed_wave)
        else:
            self._gemm(pl["frames"], self.conv0, pl["rows"][0], act=_lib.ACT_GELU, ln=self.conv_ln[0], ln_eps=1e-5, out_act=a_in,
                       k_algo=geo.conv_kernel[0], stem=True)
        # a7: conv layers 1..6 as implicit GEMMs with LayerNorm(C)+GELU fused into the epilogue
        # (the 512-wide output row lives in one block tile, so the pre-LN activations never touch HBM)
        nl = len(geo.conv_dim)
        for i in range(1, nl):
            rows = pl["rows"][i]
            if i < nl - 1:
                a_view = pl["conv_act"][i % 2].first_rows(rows)
                self._gemm(a_in, self.convs[i - 1], rows, a_rowoff=pl["conv_rowoff"][i - 1], act=_lib.ACT_GELU,
                           ln=self.conv_ln[i], ln_eps=1e-5, out_act=a_view, stem=True)     # (ln None: *-base, GELU only)
                a_in = a_view
            else:
                self._gemm(a_in, self.convs[i - 1], rows, a_rowoff=pl["conv_rowoff"][i - 1], act=_lib.ACT_GELU,
                           ln=self.conv_ln[i], ln_eps=1e-5, out_f32=pl["feat_f32"], ldo_f32=C0, stem=True)
        # a9 (its LayerNorm): the feature projection's input
        self._layernorm(pl["feat_f32"], C0, self.proj_ln, M, C0, out_act=pl["feat_act"], stem=True)

    def _wave_frames(self, pl, packed_wave: torch.Tensor) -> None:
        """ser_wave_frames: every utterance's samples normalised (``normalize``) and framed into conv layer 0's operand rows."""
        geo, fr = self.geo, pl["frames"]
        B, rows = pl["B"], pl["rows"][0]
        a = self._cmd("wave_frames")
        a.wav, a.sample_offs, a.frame_offs = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["frame_offs0"].data_ptr()
        a.B, a.k, a.stride, a.mode = B, geo.conv_kernel[0], geo.conv_stride[0], self.stem_mode
        a.out, a.out_plane_stride, a.work, a.total_rows = fr.ptr, fr.plane_stride, pl["wave_work"].data_ptr(), rows
        a.no_norm = 0 if self.normalize else 1
        a.range_flag = self._flag
        self._issue(_lib.OP_WAVE_FRAMES, a, "ser_wave_frames", input="wav", B=B, total_rows=rows)

    def _pos_stack(self, pl, states) -> None:
        """data2vec-audio's positional embedding (HF Data2VecAudioPositionalConvEmbedding): per layer j the grouped conv as an implicit
        GEMM over the zero-halo'd copy (bias added, fp32 into ``tmp``), then ser_pos_ln_v: LayerNorm (no affine) + GELU written back
        into the SAME halo'd copy at each row's halo'd position (stream order puts the GEMM's reads before the row pass's writes; the
        halo rows and the spare row the padded channels of the last group reach stay zero).  After the last layer the row pass adds the
        projection output and applies encoder.layer_norm: hidden_states[0] and layer 0's operand copy."""
        geo = self.geo
        M, D = pl["M"], geo.hidden
        G, Cg, kc, k = geo.pos_conv_groups, self.pos_cg, self.pos_kc, geo.pos_conv_kernel
        halo = pl["halo_act"]
        n = len(self.pos_stack)
        for j, lin in enumerate(self.pos_stack):
            self._gemm(halo, lin, M, a_rowoff=pl["pos_rowoff"], kc=kc, ldj=D, groups=G, a_group_stride=Cg, w_group_stride=Cg * k * kc,
                       c_group_stride=Cg, N=Cg, K=k * kc, out_f32=pl["tmp"], ldo_f32=D, k_algo=k * Cg, stem=self.pos_in_stem)
            if j + 1 < n:
                self._pos_ln(pl["tmp"], M, out_act=halo, rowmap=pl["halo_rowmap"], mode=self.stem_mode if self.pos_in_stem else self.mode)
            else:
                self._pos_ln(pl["tmp"], M, out_act=pl["xa"], mode=self.mode, residual=pl["proj_f32"], out_f32=states[0])

    def _pos_ln(self, x: torch.Tensor, rows: int, *, out_act: Optional[Act], mode: int, rowmap=None, residual=None, out_f32=None) -> None:
        """ser_pos_ln_v: the intermediate form (``residual`` None) or the last one (+ residual, encoder.layer_norm -> ``out_f32``)."""
        D = self.geo.hidden
        last = residual is not None
        a = self._cmd("pos_ln")
        a.x, a.ldx = x.data_ptr(), D
        a.out_act = None if out_act is None else out_act.ptr
        a.ldo_act = 0 if out_act is None else out_act.cols
        a.out_plane_stride = 0 if out_act is None else out_act.plane_stride
        a.out_rowmap = _ptr(rowmap)
        a.residual, a.ldr = _ptr(residual), D if last else 0
        a.g, a.b = (self.enc_ln[0].data_ptr(), self.enc_ln[1].data_ptr()) if last else (None, None)
        a.out_f32, a.ldo_f32 = _ptr(out_f32), D if last else 0
        a.eps_pos, a.eps = 1e-5, float(self.geo.layer_norm_eps)          # nn.LayerNorm(D, elementwise_affine=False): the default eps
        a.last, a.mode, a.rows, a.D = int(last), mode, rows, D
        a.range_flag = self._flag if out_act is not None else None
        self._issue(_lib.OP_POS_LN, a, "ser_pos_ln", rows=rows)

    def _groupnorm_stem(self, pl, packed_wave: torch.Tensor) -> None:
        """Conv layer 0 of the *-base form: GroupNorm(C, C) over each utterance's frames, then GELU.  ser_gn_stats_v derives the
        per-(utterance, channel) statistics from the frame moments of the waveform (one read, no pass over the conv output) and the
        conv-0 GEMM applies them in its epilogue (ser_gemm_args.gn_scale): layer 1's operand planes are its only output."""
        geo = self.geo
        B, C0 = pl["B"], geo.conv_dim[0]
        a = self._cmd("gn_stats")
        a.wav, a.sample_offs, a.frame_offs = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["frame_offs0"].data_ptr()
        a.w, a.bias, a.gamma, a.beta = self.conv0_w.data_ptr(), _ptr(self.conv0_b), self.gn0[0].data_ptr(), self.gn0[1].data_ptr()
        a.wave_stats = pl["wave_work"].data_ptr()                # what ser_wave_frames normalised the frames with (launched just before)
        a.scale, a.shift, a.stat_out, a.work = pl["gn_scale"].data_ptr(), pl["gn_shift"].data_ptr(), None, pl["gn_work"].data_ptr()
        a.B, a.C, a.k, a.stride, a.ld = B, C0, geo.conv_kernel[0], geo.conv_stride[0], C0
        a.no_norm, a.eps = 0 if self.normalize else 1, 1e-5      # nn.GroupNorm's default eps (HF WavLMGroupNormConvLayer)
        self._issue(_lib.OP_GN_STATS, a, "ser_gn_stats", input="wav", B=B)
        self._gemm(pl["frames"], self.conv0, pl["rows"][0], act=_lib.ACT_GELU, out_act=pl["conv_act"][0], k_algo=geo.conv_kernel[0],
                   stem=True, gn=(pl["gn_scale"], pl["gn_shift"], pl["frame_offs0"], B))

    def _run_post_ln_layers(self, pl, states, B: int, max_frames: int, last_state: Optional[int] = None):
        """Post-LN encoder layers (HF WavLMEncoderLayer / Wav2Vec2EncoderLayer): x -> [QKV(+gate) GEMM] -> attention -> _post_ln_tail.
        states[0] and its operand copy come from ser_layernorm (encoder.layer_norm); every LN2 but the last writes states[i+1] and the
        next copy, the last one states[L] only."""
        geo = self.geo
        M, D, L = pl["M"], geo.hidden, geo.num_layers
        wavlm = geo.family == FAMILY_WAVLM
        scale = geo.head_dim ** -0.5 * 1.4426950408889634     # q leaves multiplied by dh^-0.5 * log2(e) (exp2-domain softmax)
        if self._state_done(0, last_state):
            return
        for i, lay in enumerate(self.layers):
            last = i + 1 == L
            self._gemm(pl["xa"], lay["qkv"], M, out_act=pl["qkv"], col_scale=scale, col_scale_end=D)
            if wavlm:
                self._attention(pl["qkv"], pl["frame_offs"], B, max_frames, pl["ctx"], table=pl["table"], table_T=pl["Tmax"],
                                gru_const=lay["gate_c"])
            else:
                self._attention(pl["qkv"], pl["frame_offs"], B, max_frames, pl["ctx"])
            self._post_ln_tail(pl, lay, states[i], states[i + 1], None if last else pl["xa"])
            if not last and self._state_done(i + 1, last_state):
                return


class LongMel:
    """Whole-file Whisper features on the device (``WhisperEncoder.log_mel_long``): one grow-only fp32 buffer that holds every resident
    file's ``[n_mels][pitch]`` rows at ``bases[file]`` (float offsets, multiples of 4), with ``pitches[file]`` = the frame count rounded
    up to 4 and ``frames[file]`` = len // 160.  File indices are handed out in order and never reused; ``release(file)`` returns a file's
    span to a first-fit free list.  A buffer that runs out of room is succeeded by a larger one (the resident rows are copied on the
    stream), so ``buf`` may change between calls: launches take its address when they are issued."""

    HOP = 160

    def __init__(self, n_mels: int, device):
        self.n_mels, self.device = int(n_mels), device
        self.buf = torch.empty(0, dtype=torch.float32, device=device)
        self.top = 0
        self.bases: List[Optional[int]] = []
        self.pitches: List[int] = []
        self.frames: List[int] = []
        self.lengths: List[int] = []
        self._free: List[List[int]] = []                    # [offset, floats], ascending offsets

    def __len__(self) -> int:
        return len(self.bases)

    def _take(self, size: int) -> int:
        for k, (o, n) in enumerate(self._free):
            if n >= size:
                if n == size:
                    self._free.pop(k)
                else:
                    self._free[k] = [o + size, n - size]
                return o
        o = self.top
        if o + size > self.buf.numel():
            grown = torch.empty(max(2 * self.buf.numel(), o + size), dtype=torch.float32, device=self.device)
            grown[:o].copy_(self.buf[:o])
            self.buf = grown
        self.top = o + size
        return o

    def add(self, length: int) -> int:
        F = int(length) // self.HOP
        pitch = (F + 3) // 4 * 4
        self.bases.append(self._take(self.n_mels * pitch))
        self.pitches.append(pitch)
        self.frames.append(F)
        self.lengths.append(int(length))
        return len(self.bases) - 1

    def release(self, file: int) -> None:
        base = self.bases[file]
        if base is None:
            raise ValueError(f"file {file} was released before")
        self.bases[file] = None
        self._free.append([base, self.n_mels * self.pitches[file]])
        self._free.sort()
        merged: List[List[int]] = []
        for o, n in self._free:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1][1] += n
            else:
                merged.append([o, n])
        if merged and merged[-1][0] + merged[-1][1] == self.top:
            self.top = merged.pop()[0]
        self._free = merged

    def features(self, file: int) -> torch.Tensor:
        """[n_mels, F] view of one resident file"""
        base, pitch = self.bases[file], self.pitches[file]
        return self.buf[base: base + self.n_mels * pitch].view(self.n_mels, pitch)[:, : self.frames[file]]

    def row_table(self, rows) -> np.ndarray:
        """int64 [B][5] = base, pitch, F, seek, nf: ser_mel_window_v's row table for ``rows`` = [(file, seek, nf)]"""
        t = np.zeros((len(rows), 5), dtype=np.int64)
        for b, (f, seek, nf) in enumerate(rows):
            if not 0 <= f < len(self.bases) or self.bases[f] is None:
                raise ValueError(f"row {b}: file {f} is not resident")
            t[b] = (self.bases[f], self.pitches[f], self.frames[f], int(seek), int(nf))
        return t


class WhisperEncoder(_WaveIO, _EncoderBase):
    """Whisper encoder (log-mel front end + stem convs + pre-LN layers) on libserhip."""

    N_SAMPLES = 480000
    N_FRAMES = 3000

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "bf16", mel_filters=None):
        super().__init__(geo, device, mode)
        if geo.family != FAMILY_WHISPER:
            raise ValueError("WhisperEncoder needs a whisper geometry")
        sd = state_dict
        D = geo.hidden
        from .frontend import whisper_mel_filters
        self.mel = self._dev_f32(torch.from_numpy(whisper_mel_filters(geo.n_mels) if mel_filters is None else mel_filters))
        w1 = sd["encoder.conv1.weight"].float()
        w2 = sd["encoder.conv2.weight"].float()
        self.conv1 = self._linear(w1.permute(0, 2, 1).reshape(D, -1), sd["encoder.conv1.bias"], stem=True, name="encoder.conv1.weight")
        self.conv2 = self._linear(w2.permute(0, 2, 1).reshape(D, -1), sd["encoder.conv2.bias"], stem=True, name="encoder.conv2.weight")
        self.pos_emb = self._dev_f32(sd["encoder.embed_positions.weight"])
        self.enc_ln = self._ln_pair(sd, "encoder.layer_norm")
        self.layers = []
        for i in range(geo.num_layers):
            p = f"encoder.layers.{i}"
            self.layers.append(self._layer_weights(
                sd, p, p + ".self_attn", p + ".self_attn_layer_norm", p + ".final_layer_norm",
                p + ".fc1", p + ".fc2", k_bias=False, gate=False, index=i))        # k_proj has no bias

    def _plan(self, lengths, slot: int = 0):
        """Every Whisper shape is a function of B alone (30 s windows), so buffers are keyed by (slot, B) and a new
        batch only uploads its B+1 sample offsets."""
        lengths = tuple(int(n) for n in lengths)
        pl = self._plan_of(len(lengths), slot)
        if pl["lengths"] != lengths:
            pl["sample_offs"] = pl["tab"].begin().put64(np.concatenate([[0], np.cumsum(lengths)]))
            pl["tab"].send()
            pl["lengths"] = lengths
        return pl

    def _plan_of(self, B: int, slot: int):
        """the (slot, B) plan, built on a miss; its sample offsets are ``_plan``'s business"""
        pl = self._cache.pop((slot, B), None)
        if pl is None:
            return self._build_plan(B, slot)
        self._cache[(slot, B)] = pl                     # re-insert: the dict is kept in least-recently-USED order, the hot
        #                                                 full-batch plans of the pipeline slots are never the ones evicted
        return pl

    def _build_plan(self, B: int, slot: int):
        key_full = (slot, B)
        geo, dev = self.geo, self.device
        D, Fd, nm = geo.hidden, geo.ffn, geo.n_mels
        T2, T1 = geo.max_source_positions, self.N_FRAMES
        if T1 != 2 * T2:
            raise ValueError("max_source_positions must be 1500 (3000 mel frames / 2)")
        Tp = T1 + 2
        M = B * T2
        pl = dict(B=B, M=M, lengths=None, tab=TableBlob(B, 1, dev))
        pl["mel"] = torch.empty((B, nm, T1), dtype=torch.float32, device=dev)
        ws = lib.ser_workspace_bytes(_lib.WS_LOGMEL, B, 0, 0, 0, self.stem_mode)
        pl["work"] = torch.empty(ws, dtype=torch.uint8, device=dev)
        check(lib.ser_logmel_init(pl["work"].data_ptr(), B, _stream()), "ser_logmel_init")     # DFT twiddles: once per buffer
        pl["mel_act"] = self._new_act(B * Tp, nm, stem=True)
        pl["c1_act"] = self._new_act(B * Tp, D, zero=True, stem=True)
        b_idx = np.repeat(np.arange(B, dtype=np.int64), T1)
        t_idx = np.tile(np.arange(T1, dtype=np.int64), B)
        pl["c1_rowoff"] = torch.tensor((b_idx * Tp + t_idx) * nm // 8, dtype=torch.int32, device=dev)
        pl["c1_rowmap"] = torch.tensor(b_idx * Tp + 1 + t_idx, dtype=torch.int32, device=dev)
        b2 = np.repeat(np.arange(B, dtype=np.int64), T2)
        t2 = np.tile(np.arange(T2, dtype=np.int64), B)
        pl["c2_rowoff"] = torch.tensor((b2 * Tp + 2 * t2) * D // 8, dtype=torch.int32, device=dev)
        pl["frame_offs_host"] = [int(b * T2) for b in range(B + 1)]
        pl["frame_offs"] = torch.tensor(pl["frame_offs_host"], dtype=torch.int32, device=dev)
        pl["states"] = torch.empty((geo.num_layers + 1, M, D), dtype=torch.float32, device=dev)
        pl["first_groups"] = 2
        self._layer_buffers(pl, M, pl["first_groups"])
        if len(self._cache) >= 9:                       # three pipeline slots x (full batch, tail batch, retry of one) before anything is evicted
            self._cache.pop(next(iter(self._cache)))
        self._cache[key_full] = pl
        return pl

    def _logmel(self, pl, packed_wave: torch.Tensor) -> None:
        a = self._cmd("logmel")
        a.wav, a.sample_offs, a.mel = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), self.mel.data_ptr()
        a.out, a.work, a.B, a.n_mels = pl["mel"].data_ptr(), pl["work"].data_ptr(), pl["B"], self.geo.n_mels
        self._issue(_lib.OP_LOGMEL, a, "ser_logmel_whisper", input="wav")

    @_on_stream
    def log_mel(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0) -> torch.Tensor:
        """a16: [B, n_mels, 3000] fp32 input_features, computed on the GPU."""
        pl = self._plan(lengths, slot)
        self._logmel(pl, packed_wave)
        return pl["mel"]

    @_on_stream
    def forward(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0,
                last_state: Optional[int] = None) -> HiddenStates:
        """packed raw samples -> log-mel (a16) -> encoder (a17): the reference's processor + model.encoder calls
        (preprocess_whisper.py:48,57).  Every buffer is a function of (slot, B), so the ~170 launches are recorded once
        per plan and replayed with one ser_run call; only the waveform pointer changes from batch to batch.
        ``last_state`` = N stops after hidden state N (``--n_layer N``, preprocess_whisper.py:71)."""
        pl = self._plan(lengths, slot)
        return self._launch_or_replay(pl, pl, packed_wave, self._check_last_state(last_state))

    def _launches(self, pl, packed_wave: torch.Tensor, last_state: Optional[int] = None) -> None:
        self._logmel(pl, packed_wave)
        self._encoder_launches(pl, pl["mel"], last_state)

    @_on_stream
    def forward_features(self, input_features: torch.Tensor, lengths: Sequence[int], slot: int = 0) -> HiddenStates:
        """a17: ``model.encoder(input_features, output_hidden_states=True).hidden_states`` on caller-supplied features."""
        geo = self.geo
        pl = self._plan(lengths, slot)
        if tuple(input_features.shape) != (pl["B"], geo.n_mels, self.N_FRAMES):
            raise ValueError(f"Whisper expects input_features of shape {(pl['B'], geo.n_mels, self.N_FRAMES)}, "
                             f"got {tuple(input_features.shape)}")
        flag = self._guard_word(pl)
        self._encoder_launches(pl, input_features)
        return HiddenStates(pl["states"], pl["frame_offs_host"], range_flag=flag)

    # ------------------------------------------------------------------ long-form: whole-file features and windows of them (a37)
    def _build_long(self, cap: Dict[str, int]) -> dict:
        """tables and scratch of one ser_logmel_long_v launch: sample offsets [B + 1], bases [B] (int64), files [B][4], tiles [tiles][2] (int32)"""
        B, tiles = cap["B"], cap["tiles"]
        words = (B + 1) + B + 2 * B + tiles
        return dict(pin=Pinned(words, torch.int64), dev=torch.empty(words, dtype=torch.int64, device=self.device),
                    scratch=torch.empty(tiles + B, dtype=torch.float32, device=self.device))

    @_on_stream
    def log_mel_long(self, packed_wave: torch.Tensor, lengths: Sequence[int], into: Optional[LongMel] = None) -> LongMel:
        """HF's long-form input features (``WhisperFeatureExtractor(truncation=False)``) of B ragged files in one ser_logmel_long_v launch:
        one reflect pad at each file's own ends, len // 160 frames, one max - 8 floor per FILE.  Returns the handle (``LongMel``) that
        holds the device buffer, the bases, the pitches and the frame counts; ``into``: a handle to add the files to (the window queue
        admits files while others are resident) -- their indices are ``len(into)`` onwards."""
        lengths = [int(n) for n in lengths]
        B = len(lengths)
        if B < 1 or packed_wave.numel() != sum(lengths):
            raise ValueError("log_mel_long: one length per file, and the packed samples of exactly these files")
        for n in lengths:
            if n < 201:
                raise ValueError(f"log_mel_long: a file of {n} samples (the reflect pad of 200 needs at least 201)")
        h = into if into is not None else LongMel(self.geo.n_mels, self.device)
        if getattr(self, "_long_arenas", None) is None:
            self._long_arenas = SlotArenas(self._build_long)
            ws = lib.ser_workspace_bytes(_lib.WS_LOGMEL, 1, 0, 0, 0, self.stem_mode)
            self._long_table = torch.empty(ws, dtype=torch.uint8, device=self.device)
            check(lib.ser_logmel_init(self._long_table.data_ptr(), 1, self._s()), "ser_logmel_init")
        first = len(h)
        files = [h.add(n) for n in lengths]
        F = [h.frames[f] for f in files]
        counts = [(f + 31) // 32 for f in F]
        n_tiles = int(sum(counts))
        ar = self._long_arenas.fit(0, B=B, tiles=n_tiles)
        pin, dev = ar["pin"], ar["dev"]
        pin.wait()
        host = pin.host.numpy()
        o_offs, o_bases, o_files, o_tiles = 0, B + 1, 2 * B + 1, 4 * B + 1
        host[o_offs: o_offs + B + 1] = np.concatenate([[0], np.cumsum(lengths)])
        host[o_bases: o_bases + B] = [h.bases[f] for f in files]
        ft = np.zeros((B, 4), dtype=np.int32)
        ft[:, 0], ft[:, 1], ft[:, 3] = F, [h.pitches[f] for f in files], counts
        ft[:, 2] = np.concatenate([[0], np.cumsum(counts)[:-1]])
        host[o_files: o_files + 2 * B].view(np.int32)[:] = ft.reshape(-1)
        tt = np.empty((n_tiles, 2), dtype=np.int32)
        tt[:, 0] = np.repeat(np.arange(B, dtype=np.int32), counts)
        tt[:, 1] = np.concatenate([np.arange(c, dtype=np.int32) * 32 for c in counts])
        host[o_tiles: o_tiles + n_tiles].view(np.int32)[:] = tt.reshape(-1)
        used = o_tiles + n_tiles
        dev[:used].copy_(pin.host[:used], non_blocking=True)
        pin.sent()
        a = self._cmd("logmel_long")
        a.wav, a.sample_offs, a.sample_offs_host = packed_wave.data_ptr(), dev.data_ptr() + 8 * o_offs, pin.host.data_ptr() + 8 * o_offs
        a.mel, a.out, a.bases = self.mel.data_ptr(), h.buf.data_ptr(), dev.data_ptr() + 8 * o_bases
        a.files, a.tiles = dev.data_ptr() + 8 * o_files, dev.data_ptr() + 8 * o_tiles
        a.table, a.scratch = self._long_table.data_ptr(), ar["scratch"].data_ptr()
        a.B, a.n_mels, a.n_tiles, a.max_pitch = B, self.geo.n_mels, n_tiles, max(h.pitches[f] for f in files)
        self._issue(_lib.OP_LOGMEL_LONG, a, "ser_logmel_long_v")
        assert files[0] == first
        return h

    def _mel_window(self, pl, win) -> None:
        a = self._cmd("mel_window")
        a.src, a.rows, a.rows_host, a.out = win["src"], win["rows"].data_ptr(), win["tab"].host.data_ptr(), pl["mel"].data_ptr()
        a.B, a.n_mels = pl["B"], self.geo.n_mels
        self._issue(_lib.OP_MEL_WINDOW, a, "ser_mel_window_v", input="src")

    @_on_stream
    def forward_windows(self, handle: LongMel, rows: Sequence[tuple], slot: int = 0, last_state: Optional[int] = None) -> HiddenStates:
        """The encoder over B windows of resident files: ``rows`` = [(file, seek, nf)], window b = the file's features at
        [seek, seek + nf) followed by 3000 - nf columns of 0.0 (HF's ``_get_input_segment``).  One command list per (slot, B) -- the gather
        into the plan's ``mel``, then ``forward``'s encoder launches -- recorded once and replayed like ``forward``'s; from window to window
        only the row table (and, after the handle grew, its buffer's address) changes."""
        B = len(rows)
        pl = self._plan_of(B, slot)
        win = pl.get("win")
        if win is None:
            win = pl["win"] = dict(tab=TableBlob(5 * B, 1, self.device))
        win["rows"] = win["tab"].begin().put64(handle.row_table(rows).reshape(-1))
        win["tab"].send()
        win["src"] = handle.buf.data_ptr()
        flag = self._guard_word(pl)
        last_state = self._check_last_state(last_state)

        def launch(last):
            self._mel_window(pl, win)
            self._encoder_launches(pl, pl["mel"], last)
        self._replay((win,), {}, launch, win["src"], last_state)
        return HiddenStates(pl["states"], pl["frame_offs_host"], None if last_state is None else last_state + 1, range_flag=flag,
                            frame_offs_dev=pl.get("frame_offs"))

    def _pack_act(self, pl, input_features: torch.Tensor) -> None:
        """ser_pack_act: the [B, n_mels, 3000] features as conv1's operand rows (channels last, a zero halo row before and after each utterance)."""
        ma, nm = pl["mel_act"], self.geo.n_mels
        a = self._cmd("pack_act")
        a.x, a.out, a.ldo, a.out_plane_stride = input_features.data_ptr(), ma.ptr, nm, ma.plane_stride
        a.B, a.C, a.T, a.halo, a.mode = pl["B"], nm, self.N_FRAMES, 1, self.stem_mode
        a.range_flag = self._flag
        self._issue(_lib.OP_PACK_ACT, a, "ser_pack_act")

    def _encoder_launches(self, pl, input_features: torch.Tensor, last_state: Optional[int] = None) -> None:
        geo = self.geo
        B, M, D = pl["B"], pl["M"], geo.hidden
        T1, T2 = self.N_FRAMES, geo.max_source_positions
        self._pack_act(pl, input_features)
        # stem: gelu(conv1 k3 p1), gelu(conv2 k3 s2 p1) + embed_positions -> hidden_states[0]
        self._gemm(pl["mel_act"], self.conv1, B * T1, a_rowoff=pl["c1_rowoff"], act=_lib.ACT_GELU, out_act=pl["c1_act"],
                   out_rowmap=pl["c1_rowmap"], stem=True)
        states = pl["states"]
        self._gemm(pl["c1_act"], self.conv2, M, a_rowoff=pl["c2_rowoff"], act=_lib.ACT_GELU, residual=self.pos_emb,
                   ldr=D, res_row_mod=T2, out_f32=states[0], ldo_f32=D, stem=True)
        self._run_layers(pl, states, pl["first_groups"], B, T2, last_state)


class _TextEncoderBase(_EncoderBase):
    """What the RoBERTa and DeBERTa encoders share: post-LN layers, ``forward``'s input checks and the plans, one per (slot, B, T)."""

    def __init__(self, geo: EncoderGeometry, device, mode: str):
        super().__init__(geo, device, mode, post_ln=True)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, slot: int = 0) -> HiddenStates:
        """``model(input_ids, attention_mask, output_hidden_states=True).hidden_states`` (preprocess_roberta.py /
        preprocess_deroberta.py:57,68)."""
        B, T = input_ids.shape
        if attention_mask.shape != input_ids.shape:
            raise ValueError("attention_mask must have the shape of input_ids")
        if int(input_ids.min()) < 0 or int(input_ids.max()) >= self.geo.vocab_size:
            raise ValueError("token id outside the vocabulary")
        mask = attention_mask.to(torch.int64).cpu()
        klen = mask.sum(dim=1)
        if not torch.equal(mask, (torch.arange(T)[None, :] < klen[:, None]).to(torch.int64)) or int(klen.min()) < 1:
            raise ValueError("attention_mask must be right-padded with at least one valid token per sequence")
        ids = input_ids.to(device=self.device, dtype=torch.int32).contiguous()
        return self.forward_device(ids, klen.to(device=self.device, dtype=torch.int32), slot)

    def _plan(self, B: int, T: int, slot: int = 0):
        key = (slot, B, T)
        if key in self._cache:
            return self._cache[key]
        geo, dev = self.geo, self.device
        M = B * T
        pl = dict(B=B, T=T, M=M)
        pl["frame_offs_host"] = [b * T for b in range(B + 1)]
        pl["frame_offs"] = torch.tensor(pl["frame_offs_host"], dtype=torch.int32, device=dev)
        pl["states"] = torch.empty((geo.num_layers + 1, M, geo.hidden), dtype=torch.float32, device=dev)
        self._post_ln_buffers(pl, M, 3 * geo.hidden)
        self._own_buffers(pl)
        if len(self._cache) >= 4:
            self._cache.pop(next(iter(self._cache)))
        self._cache[key] = pl
        return pl

    def _own_buffers(self, pl) -> None:
        """buffers of a plan beyond the shared set"""


class TextEncoder(_TextEncoderBase):
    """RoBERTa text encoder (next row 8f-1: preprocessing/preprocess_roberta.py) on the same kernels:
    embeddings + L post-LayerNorm BERT layers.  ``forward(input_ids [B,T], attention_mask [B,T])`` returns
    L+1 states per sequence, ALL T rows each (the reference saves the padded positions too); padded KEYS
    are excluded through per-sequence key lengths (tokenizer padding="max_length" pads on the right)."""

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "bf16"):
        super().__init__(geo, device, mode)
        if geo.family != FAMILY_ROBERTA:
            raise ValueError("TextEncoder needs a roberta geometry")
        sd = state_dict
        self.wemb = self._dev_f32(sd["embeddings.word_embeddings.weight"])
        self.pemb = self._dev_f32(sd["embeddings.position_embeddings.weight"])
        self.temb = self._dev_f32(sd["embeddings.token_type_embeddings.weight"][0])
        self.emb_ln = self._ln_pair(sd, "embeddings.LayerNorm")
        self.layers = []
        for i in range(geo.num_layers):
            p = f"encoder.layer.{i}"
            a = p + ".attention.self"
            self.layers.append(self._post_ln_layer_weights(
                sd, a + ".query", a + ".key", a + ".value", p + ".attention.output.dense", p + ".attention.output.LayerNorm",
                p + ".intermediate.dense", p + ".output.dense", p + ".output.LayerNorm"))

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, slot: int = 0) -> HiddenStates:
        """``model(input_ids, attention_mask, output_hidden_states=True).hidden_states`` (preprocess_roberta.py:57,68)."""
        T, geo = input_ids.shape[-1], self.geo
        if T + geo.pad_token_id + 1 > geo.max_positions:
            # position ids run up to T + padding_idx (HF modeling_roberta.py:142): the table must hold them
            raise ValueError(f"{T} tokens need {T + geo.pad_token_id + 1} position embeddings, the model has {geo.max_positions}")
        return super().forward(input_ids, attention_mask, slot)

    @_on_stream
    def forward_device(self, ids: torch.Tensor, key_lens: torch.Tensor, slot: int = 0) -> HiddenStates:
        """Same as ``forward`` with inputs already on the device (int32 ids [B,T], int32 key lengths [B]):
        no host synchronisation, so it can be captured into a hipGraph."""
        geo = self.geo
        B, T = ids.shape
        pl = self._plan(B, T, slot)
        flag = self._guard_word(pl)
        M, D = pl["M"], geo.hidden
        states = pl["states"]
        xa = pl["xa"]
        check(lib.ser_embed_ln_flagged(ids.data_ptr(), self.wemb.data_ptr(), self.pemb.data_ptr(), self.temb.data_ptr(),
                                       self.emb_ln[0].data_ptr(), self.emb_ln[1].data_ptr(), float(geo.layer_norm_eps),
                                       states[0].data_ptr(), xa.ptr, xa.plane_stride, self.mode, B, T, D, geo.pad_token_id,
                                       self._flag, _stream()), "ser_embed_ln_flagged")
        scale = geo.head_dim ** -0.5 * 1.4426950408889634
        for i, lay in enumerate(self.layers):
            self._gemm(xa, lay["qkv"], M, out_act=pl["qkv"], col_scale=scale, col_scale_end=D)
            self._attention(pl["qkv"], pl["frame_offs"], B, T, pl["ctx"], key_lens=key_lens)
            self._post_ln_tail(pl, lay, states[i], states[i + 1], xa)
        return HiddenStates(states, pl["frame_offs_host"], range_flag=flag)


def _deberta_log_bucket(rel: torch.Tensor, bucket_size: int, max_position: int) -> torch.Tensor:
    """Signed distance -> bucket, in the float32 arithmetic HF uses (modeling_deberta_v2.py make_log_bucket_position):
    identity inside +-bucket_size/2, logarithmic beyond.  O(T) host work per sequence length; the kernels only see the
    resulting integer columns."""
    mid = bucket_size // 2
    sign = torch.sign(rel)
    inside = (rel < mid) & (rel > -mid)
    a = torch.where(inside, torch.full_like(rel, mid - 1), rel.abs()).to(torch.float32)
    logp = torch.ceil(torch.log(a / mid) / math.log((max_position - 1) / mid) * (mid - 1)) + mid
    return torch.where(a <= mid, rel.to(torch.float32), logp * sign).to(torch.long)


class DebertaEncoder(_TextEncoderBase):
    """DeBERTa-v2/v3 text encoder (preprocessing/preprocess_deroberta.py builds it with AutoModel) in its v3
    configuration: LayerNorm-ed word embeddings (no absolute positions / token types), L post-LayerNorm blocks with
    disentangled attention.  The relative-position side is input independent, so it is folded at load: LayerNorm of the
    relative embeddings and their projection through every layer's (shared) query / key weights.  Per layer the device
    then runs the packed QKV GEMM, two grouped GEMMs (content queries x position keys, content keys x position queries,
    restricted to the relative rows a T-token sequence can reach), ``ser_deberta_attention``, and the same post-LN
    output / feed-forward GEMMs as the RoBERTa encoder.  Same call surface as ``TextEncoder``."""

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "bf16"):
        super().__init__(geo, device, mode)
        if geo.family != "deberta":
            raise ValueError("DebertaEncoder needs a deberta geometry")
        if geo.head_dim != 64:
            raise ValueError("DeBERTa path: head dim must be 64 (K of the position GEMMs; deberta-v3 base/large have 64)")
        sd = state_dict
        D, span = geo.hidden, geo.position_buckets
        self.wemb = self._dev_f32(sd["embeddings.word_embeddings.weight"])
        self.emb_ln = self._ln_pair(sd, "embeddings.LayerNorm")
        rel = sd["encoder.rel_embeddings.weight"][: 2 * span].double()
        rel = torch.nn.functional.layer_norm(rel, (D,), sd["encoder.LayerNorm.weight"].double(), sd["encoder.LayerNorm.bias"].double(),
                                             geo.layer_norm_eps)
        self.layers = []
        for i in range(geo.num_layers):
            p = f"encoder.layer.{i}"
            a = p + ".attention.self"
            wq, wk = sd[a + ".query_proj.weight"].double(), sd[a + ".key_proj.weight"].double()
            bq, bk = sd[a + ".query_proj.bias"].double(), sd[a + ".key_proj.bias"].double()
            lay = self._post_ln_layer_weights(
                sd, a + ".query_proj", a + ".key_proj", a + ".value_proj", p + ".attention.output.dense", p + ".attention.output.LayerNorm",
                p + ".intermediate.dense", p + ".output.dense", p + ".output.LayerNorm")
            lay["pos_q"], lay["pos_k"] = (rel @ wq.T + bq).float(), (rel @ wk.T + bk).float()     # [2 span, D] fp32, host: windows cut per T
            self.layers.append(lay)
        # deberta-v2 xlarge / xxlarge: ConvLayer after layer 0 (HF modeling_deberta_v2.py ConvLayer) as an implicit-conv GEMM
        self.text_conv = None
        if geo.text_conv_kernel:
            if geo.text_conv_kernel != 3:
                raise ValueError("DeBERTa ConvLayer: kernel size 3 (deberta-v2-xlarge / xxlarge) is what is built")
            wc = sd["encoder.conv.conv.weight"].float()                                    # [out, in, tap]
            self.text_conv = dict(lin=self._linear(wc.permute(0, 2, 1).reshape(D, 3 * D), sd["encoder.conv.conv.bias"], name="encoder.conv.conv.weight"),
                                  ln=self._ln_pair(sd, "encoder.conv.LayerNorm"))
        self._windows: Dict[int, dict] = {}

    def _window(self, T: int):
        """Everything that depends on the sequence length only: which relative rows are reachable, the column of every
        signed distance inside that window, and each layer's position keys / queries cut to it as [H, Nr, dh] GEMM weights."""
        if T in self._windows:
            return self._windows[T]
        geo = self.geo
        span, H, dh = geo.position_buckets, geo.heads, geo.head_dim
        d = torch.arange(-(T - 1), T)
        bucket = _deberta_log_bucket(d, span, geo.max_positions)
        c2p_row = torch.clamp(bucket + span, 0, 2 * span - 1)            # row of pos_k for distance d = q - k
        p2c_row = torch.clamp(-bucket + span, 0, 2 * span - 1)           # row of pos_q for distance d = k - q
        lo = int(min(c2p_row.min(), p2c_row.min()))
        hi = int(max(c2p_row.max(), p2c_row.max())) + 1
        Nr = min(2 * span, (hi - lo + 7) // 8 * 8)                       # GEMM N: a multiple of 8 (2 span is one)
        lo = max(0, min(lo, 2 * span - Nr))                              # ... so slide the window back inside the table
        w = dict(Nr=Nr, lo=lo,
                 c2p_col=(c2p_row - lo).to(torch.int32).to(self.device), p2c_col=(p2c_row - lo).to(torch.int32).to(self.device), layers=[])
        for lay in self.layers:
            cut = lambda m: m[lo:lo + Nr].reshape(Nr, H, dh).permute(1, 0, 2).reshape(H * Nr, dh)     # noqa: E731
            # ONE grouped GEMM gives both position terms: the k columns follow the q columns in the packed projection, so
            # group g < H reads query head g and group H + h reads key head h with the same column step dh; the weights are
            # the position keys of every head followed by the position queries of every head
            w["layers"].append(self._linear(torch.cat([cut(lay["pos_k"]), cut(lay["pos_q"])], 0), None))
        self._windows[T] = w
        return w

    def _own_buffers(self, pl) -> None:
        geo, dev = self.geo, self.device
        B, T, M, D = pl["B"], pl["T"], pl["M"], geo.hidden
        win = pl["win"] = self._window(T)
        pl["posterms"] = torch.empty((M, 2 * geo.heads * win["Nr"]), dtype=torch.float32, device=dev)   # [c2p of every head | p2c of every head]
        pl["bias2d"] = torch.zeros((B, geo.heads, T, (T + 63) // 64 * 64), dtype=torch.float32, device=dev)   # dense c2p + p2c bias
        if self.text_conv is not None:
            pl["conv_in"] = self._new_act(B * (T + 2), D, zero=True)                       # [0][tokens of sequence b][0] per sequence
            b_idx = np.repeat(np.arange(B, dtype=np.int64), T)
            t_idx = np.tile(np.arange(T, dtype=np.int64), B)
            pl["conv_rowoff"] = torch.tensor((b_idx * (T + 2) + t_idx) * D // 8, dtype=torch.int32, device=dev)   # tap 0 = token t-1

    @_on_stream
    def forward_device(self, ids: torch.Tensor, key_lens: torch.Tensor, slot: int = 0) -> HiddenStates:
        geo = self.geo
        B, T = ids.shape
        pl = self._plan(B, T, slot)
        flag = self._guard_word(pl)
        M, D, H, dh = pl["M"], geo.hidden, geo.heads, geo.head_dim
        win = pl["win"]
        Nr = win["Nr"]
        states, xa, qkv = pl["states"], pl["xa"], pl["qkv"]
        st = self._s()
        check(lib.ser_embed_ln_masked_flagged(ids.data_ptr(), self.wemb.data_ptr(), self.emb_ln[0].data_ptr(), self.emb_ln[1].data_ptr(),
                                              float(geo.layer_norm_eps), key_lens.data_ptr(), states[0].data_ptr(), xa.ptr,
                                              xa.plane_stride, self.mode, B, T, D, self._flag, st), "ser_embed_ln_masked_flagged")
        # scores run in the exp2 domain: q leaves the projection multiplied by (3 dh)^-0.5 * log2(e), so the content term and the
        # content -> position term (a product with q) arrive scaled; the position -> content term (a product with k) is scaled
        # by ser_deberta_bias.  (HF: (Qc Kc^T + c2p + p2c) / sqrt(3 dh), modeling_deberta_v2.py DisentangledSelfAttention.)
        s2 = (3.0 * dh) ** -0.5 * 1.4426950408889634
        bias2d = pl["bias2d"]
        for i, lay in enumerate(self.layers):
            self._gemm(xa, lay["qkv"], M, out_act=qkv, col_scale=s2, col_scale_end=D)
            # content -> position (q x position keys) and position -> content (k x position queries) terms: one grouped GEMM,
            # group = (term, head), K = dh
            pt = pl["posterms"]
            self._gemm(qkv, win["layers"][i], M, groups=2 * H, a_group_stride=dh, w_group_stride=Nr * dh, c_group_stride=Nr,
                       N=Nr, K=dh, out_f32=pt, ldo_f32=2 * H * Nr)
            # dense bias of every (sequence, head) from the two gathers, then the matrix-core attention kernel of the speech
            # encoders with it (the 80-token VALU kernel ser_deberta_attention was a third of the step)
            check(lib.ser_deberta_bias(pt.data_ptr(), pt.data_ptr() + 4 * H * Nr, 2 * H * Nr, Nr, win["c2p_col"].data_ptr(),
                                       win["p2c_col"].data_ptr(), key_lens.data_ptr(), bias2d.data_ptr(), bias2d.shape[-1],
                                       B, T, H, float(s2), st), "ser_deberta_bias")
            self._attention(qkv, pl["frame_offs"], B, T, pl["ctx"], key_lens=key_lens, bias2d=bias2d)
            self._post_ln_tail(pl, lay, states[i], states[i + 1], xa)
            if i == 0 and self.text_conv is not None:
                # ConvLayer: LN(layer-0 output + gelu(Conv1d_k3(embeddings))) with padded rows zero.  (HF zeroes the padded
                # rows of the conv output before the activation too; gelu(0) = 0 and those rows are zeroed at the end anyway.)
                ci = pl["conv_in"]
                check(lib.ser_pack_rows_flagged(states[0].data_ptr(), D, B, T, D, 1, ci.ptr, D, ci.plane_stride, self.mode,
                                                self._flag, st), "ser_pack_rows_flagged")
                self._gemm(ci, self.text_conv["lin"], M, a_rowoff=pl["conv_rowoff"], kc=D, ldj=D, K=3 * D, act=_lib.ACT_GELU,
                           residual=states[1], ldr=D, out_f32=pl["tmp"], ldo_f32=D)
                self._layernorm(pl["tmp"], D, self.text_conv["ln"], M, D, out_f32=states[1], out_act=xa)
                check(lib.ser_zero_padded_rows(states[1].data_ptr(), D, xa.ptr, D, xa.plane_stride, self.mode, key_lens.data_ptr(),
                                               B, T, D, st), "ser_zero_padded_rows")
        return HiddenStates(states, pl["frame_offs_host"], range_flag=flag)


def mean_last4(hs: HiddenStates) -> torch.Tensor:
    """``--use_average y``: mean of the last four states (preprocess_speech.py:52-63), on the GPU."""
    s = hs.states
    if getattr(hs, "computed", s.shape[0]) < s.shape[0]:
        raise IndexError("mean of the last four states needs the full forward (this one stopped early: last_state)")
    out = torch.empty_like(s[0])
    n = out.numel()
    check(lib.ser_mean4(s[-4].data_ptr(), s[-3].data_ptr(), s[-2].data_ptr(), s[-1].data_ptr(), out.data_ptr(), n, _stream()),
          "ser_mean4")
    return out


class _HeadBase:
    """what the device heads share: the per-step timing of ``forward``"""
    trace: Optional[list] = None          # when a list: (name, start event, end event) per step (tools/pool_head_bench.py, fusion_head_bench.py)

    def _step(self, name: str, fn) -> None:
        if self.trace is None:
            fn()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.trace.append((name, e0, e1))


def _head_offs(tab: TableBlob, frame_offs) -> torch.Tensor:
    """the frame offsets of a batch that came without them on the device, through the slot's blob"""
    offs = tab.begin().put32(frame_offs)
    tab.send()
    return offs


class PoolHead(_HeadBase):
    """The organiser baseline's utterance-level tail on the device (benchmark/train_eval_files/eval_cat_ser.py:164-177):
    ``last_hidden_state`` -> AttentiveStatisticsPooling -> EmotionRegression -> ``[B, n_out]`` logits, so a waveform -> prediction run
    brings ``n_out`` floats per utterance back instead of ``[T, D]``.  Built from a speech encoder (its device and numerics mode) and the
    two state dicts of ``final_pool.pt`` / ``final_ser.pt``.  ``forward`` enqueues five steps on the current stream, after the
    encoder's recorded forward (no command-list op, the tapes stay as they are):
      operand copy of ``hs.states[-1]`` (ser_pack_rows_flagged) -> ser_gemm with sap_linear (bias epilogue, fp32 out)
      -> ser_asp_pool_v (scores, weighted moments) -> ser_mlp_head_v (hidden units, LayerNorm / ReLU / outputs).
    GEMM operand format: bf16 in mode "bf16", bf16 hi + lo in "fp32x", fp16 hi + lo in every other mode -- the product feeds tanh and
    then a softmax over the frames, where single-product rounding is not benign."""

    def __init__(self, enc: "_EncoderBase", pool_sd, ser_sd):
        geo = enc.geo
        if geo.family == FAMILY_WHISPER or not isinstance(enc, SpeechEncoder):
            raise ValueError("PoolHead runs behind the speech encoders (WavLM / wav2vec2 / HuBERT / data2vec-audio), not Whisper or text")
        D = geo.hidden
        if D % 64:
            raise ValueError(f"PoolHead needs a hidden width that is a multiple of 64 (ser_gemm's K rule), got {D}")
        self.enc, self.D, self.device = enc, D, enc.device
        self.op_mode = _operand_mode(enc.mode_name)
        w, b, a = pool_sd["sap_linear.weight"], pool_sd["sap_linear.bias"], pool_sd["attention"]
        if tuple(w.shape) != (D, D) or tuple(b.shape) != (D,) or a.numel() != D:
            raise ValueError(f"pooling weights do not match hidden width {D}: sap_linear.weight {tuple(w.shape)}, attention {tuple(a.shape)}")
        self.sap = enc._linear(w, b, mode=self.op_mode, name="final_pool.pt sap_linear.weight")
        self.att = enc._dev_f32(a.reshape(D))
        w1, w2 = ser_sd["fc.0.0.weight"], ser_sd["out.0.weight"]
        self.H, self.n_out = int(w1.shape[0]), int(w2.shape[0])
        if w1.shape[1] != 2 * D or w2.shape[1] != self.H or not 1 <= self.n_out <= 8 or 2 * D > 4096:
            raise ValueError(f"head weights do not match: fc.0.0.weight {tuple(w1.shape)} (expected [H, {2 * D}]), out.0.weight "
                             f"{tuple(w2.shape)} (expected [n_out <= 8, H])")
        self.w1, self.b1 = enc._dev_f32(w1), enc._dev_f32(ser_sd["fc.0.0.bias"])
        self.ln_g, self.ln_b = enc._dev_f32(ser_sd["fc.0.1.weight"]), enc._dev_f32(ser_sd["fc.0.1.bias"])
        self.w2, self.b2 = enc._dev_f32(w2), enc._dev_f32(ser_sd["out.0.bias"])
        self.ln_eps = 1e-5                                        # nn.LayerNorm's default (ser.py builds it without an eps)
        self._bufs = SlotArenas(self._build_buffers)

    def _build_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one pipeline slot (slots run on streams of their own, so they share nothing)"""
        M, B, D, dev = cap["M"], cap["B"], self.D, self.device
        return dict(xa=Act(M, D, _PLANES[self.op_mode], dev, dtype=_DTYPE[self.op_mode]),
                    hlin=torch.empty((M, D), dtype=torch.float32, device=dev),
                    scores=torch.empty(M, dtype=torch.float32, device=dev),
                    pooled=torch.empty((B, 2 * D), dtype=torch.float32, device=dev),
                    hidden=torch.empty((B, self.H), dtype=torch.float32, device=dev),
                    out=torch.empty((B, self.n_out), dtype=torch.float32, device=dev), tab=TableBlob(B, 1, dev))

    def forward(self, hs: HiddenStates, slot: int = 0) -> torch.Tensor:
        """``[B, n_out]`` fp32 logits on the device (a view of the slot's buffer: valid until the slot's next ``forward``).  The range
        guard of the fp16 operand copy reports into ``hs.range_flag``, the word the encoder's forward used; ``hs.states`` is only read."""
        if hs.computed != hs.states.shape[0]:
            raise IndexError("the head needs the last hidden state (run the forward without last_state)")
        x = hs.states[-1]
        M, B, D = int(hs.frame_offs[-1]), hs.batch, self.D
        if x.shape[0] != M or x.shape[1] != D or x.stride(0) != D:
            raise ValueError("hidden states do not match the head's width")
        bf = self._bufs.fit(slot, M=M, B=B)
        st = _stream()
        offs = hs.frame_offs_dev if hs.frame_offs_dev is not None else _head_offs(bf["tab"], hs.frame_offs)
        xa = bf["xa"].first_rows(M)
        flag = hs.range_flag.data_ptr() if (hs.range_flag is not None and self.op_mode == _lib.MODE_FP16X) else None
        self._step("pack", lambda: check(lib.ser_pack_rows_flagged(x.data_ptr(), D, 1, M, D, 0, xa.ptr, D, xa.plane_stride, self.op_mode,
                                                                    flag, st), "ser_pack_rows_flagged"))
        self._step("gemm", lambda: self.enc._gemm(xa, self.sap, M, out_f32=bf["hlin"], ldo_f32=D, mode=self.op_mode))
        p = _lib.AspPoolArgs()
        p.x, p.ldx, p.hlin, p.ldh, p.a = x.data_ptr(), D, bf["hlin"].data_ptr(), D, self.att.data_ptr()
        p.frame_offs, p.scores, p.out, p.ldo = offs.data_ptr(), bf["scores"].data_ptr(), bf["pooled"].data_ptr(), 2 * D
        p.B, p.D, p.rows, p.max_frames = B, D, M, max(hs.frames(b) for b in range(B))
        self._step("asp_pool", lambda: check(lib.ser_asp_pool_v(C.byref(p), st), "ser_asp_pool_v"))
        h = _lib.MlpHeadArgs()
        h.p, h.ldp, h.W1, h.b1, h.gamma, h.beta = bf["pooled"].data_ptr(), 2 * D, self.w1.data_ptr(), self.b1.data_ptr(), self.ln_g.data_ptr(), self.ln_b.data_ptr()
        h.W2, h.b2, h.hidden, h.out, h.eps = self.w2.data_ptr(), self.b2.data_ptr(), bf["hidden"].data_ptr(), bf["out"].data_ptr(), self.ln_eps
        h.B, h.K, h.H, h.n_out = B, 2 * D, self.H, self.n_out
        self._step("mlp_head", lambda: check(lib.ser_mlp_head_v(C.byref(h), st), "ser_mlp_head_v"))
        return bf["out"][:B]


class ClassifierHead(_HeadBase):
    """The head of the hub's audio-classification checkpoints on the device (HF WavLMForSequenceClassification.forward and its five twins):
    ``hidden_states`` -> softmax(layer_weights)-weighted sum (``use_weighted_layer_sum``; else the last state) -> projector -> mean over
    the utterance's frames -> classifier -> ``[B, num_labels]`` logits.  Projector and mean commute, so ``forward`` enqueues two steps on
    the current stream behind the encoder's recorded forward (no command-list op, the tapes stay as they are):
      ser_layer_pool_v (one pass over the fp32 states: [B, D] weighted frame means) -> ser_cls_tail_v (projector and classifier per row).
    Both read fp32 and sum in float64: no operand copies, so no range guard.  Behind Whisper the utterance's frames are the whole
    1 500-row window, HF's unmasked mean.  ``head_sd``: the tensors of ``weights.split_classifier_head``; ``spec``: ``config.ClassifierSpec``."""

    def __init__(self, enc: "_EncoderBase", head_sd, spec):
        from .weights import check_classifier_head
        if not isinstance(enc, (SpeechEncoder, W2vBertEncoder, WhisperEncoder)):
            raise ValueError("ClassifierHead runs behind the speech, w2v-BERT and Whisper encoders")
        geo = enc.geo
        D, L1 = geo.hidden, geo.num_layers + 1
        self.enc, self.D, self.device = enc, D, enc.device
        self.proj, self.n_out, self.weighted = int(spec.classifier_proj_size), int(spec.num_labels), bool(spec.use_weighted_layer_sum)
        if D % 4:
            raise ValueError(f"ClassifierHead needs a hidden width that is a multiple of 4 (16-byte loads), got {D}")
        if not 1 <= self.proj <= _lib.CLS_TAIL_MAX or not 1 <= self.n_out <= _lib.CLS_TAIL_MAX:
            raise ValueError(f"classifier_proj_size {self.proj} / num_labels {self.n_out}: ser_cls_tail_v takes 1..{_lib.CLS_TAIL_MAX} each")
        check_classifier_head(head_sd, D, self.proj, self.n_out, L1, self.weighted)
        self.P, self.bp = enc._dev_f32(head_sd["projector.weight"]), enc._dev_f32(head_sd["projector.bias"])
        self.C, self.bc = enc._dev_f32(head_sd["classifier.weight"]), enc._dev_f32(head_sd["classifier.bias"])
        # softmax(layer_weights), once, in float64 from the fp32 parameter
        w = torch.softmax(head_sd["layer_weights"].detach().to(torch.float32).double(), dim=-1) if self.weighted else torch.ones(1, dtype=torch.float64)
        self.n_states = int(w.numel())
        self.w = w.contiguous().to(self.device)
        self._bufs = SlotArenas(self._build_buffers)

    def _build_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one pipeline slot (slots run on streams of their own, so they share nothing); ``work``: float64 words of ser_layer_pool_v"""
        B, dev = cap["B"], self.device
        return dict(work=torch.empty(cap["work"], dtype=torch.float64, device=dev),
                    pooled=torch.empty((B, self.D), dtype=torch.float32, device=dev),
                    out=torch.empty((B, self.n_out), dtype=torch.float32, device=dev), tab=TableBlob(B, 1, dev))

    def forward(self, hs: HiddenStates, slot: int = 0) -> torch.Tensor:
        """``[B, num_labels]`` fp32 logits on the device (a view of the slot's buffer: valid until the slot's next ``forward``);
        ``hs.states`` is only read."""
        if hs.computed < len(hs):
            raise IndexError(f"the head needs {'every hidden state' if self.weighted else 'the last hidden state'} (run the forward without "
                             f"last_state: states 0..{hs.computed - 1} of {len(hs)} were computed)")
        s = hs.states
        M, B, D = int(hs.frame_offs[-1]), hs.batch, self.D
        if s.dim() != 3 or s.shape[0] != self.enc.geo.num_layers + 1 or s.shape[2] != D or s.stride(2) != 1 or s.shape[1] < M \
                or s.dtype != torch.float32:
            raise ValueError(f"hidden states {tuple(s.shape)} do not match the head ({self.enc.geo.num_layers + 1} states of width {D}, {M} rows)")
        max_frames = max(hs.frames(b) for b in range(B))
        chunks = -(-max_frames // _lib.LAYER_POOL_FC)
        bf = self._bufs.fit(slot, B=B, work=B * chunks * self.D)
        st = _stream()
        offs = hs.frame_offs_dev if hs.frame_offs_dev is not None else _head_offs(bf["tab"], hs.frame_offs)
        offs_host = (C.c_int32 * (B + 1))(*hs.frame_offs)
        first = s if self.weighted else s[-1:]
        p = _lib.LayerPoolArgs()
        p.s, p.state_stride, p.lds, p.w = first.data_ptr(), s.stride(0), s.stride(1), self.w.data_ptr()
        p.frame_offs, p.frame_offs_host = offs.data_ptr(), C.cast(offs_host, C.c_void_p)
        p.work, p.work_elems, p.out, p.ldo = bf["work"].data_ptr(), bf["work"].numel(), bf["pooled"].data_ptr(), D
        p.n_states, p.B, p.D, p.rows, p.max_frames = self.n_states, B, D, M, max_frames
        self._step("layer_pool", lambda: check(lib.ser_layer_pool_v(C.byref(p), st), "ser_layer_pool_v"))
        t = _lib.ClsTailArgs()
        t.pooled, t.ldp, t.P, t.bp, t.C, t.bc = bf["pooled"].data_ptr(), D, self.P.data_ptr(), self.bp.data_ptr(), self.C.data_ptr(), self.bc.data_ptr()
        t.out, t.ldo, t.B, t.D, t.proj, t.n_labels = bf["out"].data_ptr(), self.n_out, B, D, self.proj, self.n_out
        self._step("cls_tail", lambda: check(lib.ser_cls_tail_v(C.byref(t), st), "ser_cls_tail_v"))
        return bf["out"][:B]


def _pad_to(n: int, m: int) -> int:
    return -(-int(n) // m) * m


class XVectorHead(_HeadBase):
    """The x-vector head of the hub's speaker-verification checkpoints on the device (HF WavLMForXVector.forward and its wav2vec2 /
    data2vec-audio / w2v-BERT twins): ``hidden_states`` -> softmax(layer_weights)-weighted sum (``use_weighted_layer_sum``; else the last
    state) -> projector -> ReLU TDNN layers (dilated, unpadded: T shrinks) -> statistics pooling (mean | unbiased std) ->
    feature_extractor (``embeddings``) -> classifier (``logits``).  A ReLU follows the projector, so nothing commutes with the mean and
    the [T, D] mix is formed.  ``forward`` enqueues on the current stream behind the encoder's recorded forward (no command-list op, the
    tapes stay as they are):
      ser_layer_mix_v (the mix as the projector's operand) -> ser_gemm (projector, operand out)
      -> per TDNN layer: ser_ragged_index (tap-0 row of every output row) -> ser_gemm (kc = the padded input width, ldj = dilation x
         pitch, fp32 out, rows packed at the layer's own offsets) -> ser_act_rows_v(relu) (the next operand; not after the last layer)
      -> ser_stat_pool_v (relu on read) -> ser_xvec_tail_v.
    Every utterance alone: no window crosses an utterance, every sum's order depends on the utterance alone.  Widths ser_gemm does not
    take are zero-padded at load -- a layer's input width to a multiple of 64 (zero weight columns, and the producer's zero weight rows
    and biases make the operand's padding columns exact zeros), the last layer's output width to a multiple of 8 -- and the statistics
    read the true width only.  GEMM operand format: bf16 in mode "bf16", bf16 hi + lo in "fp32x", fp16 hi + lo otherwise; the fp16
    copies report to ``hs.range_flag``.  ``head_sd``: the tensors of ``weights.split_xvector_head``; ``spec``: ``config.XVectorSpec``."""

    def __init__(self, enc: "_EncoderBase", head_sd, spec):
        from .weights import check_xvector_head
        if not isinstance(enc, (SpeechEncoder, W2vBertEncoder)):
            raise ValueError("XVectorHead runs behind the speech and w2v-BERT encoders")
        geo = enc.geo
        D, L1 = geo.hidden, geo.num_layers + 1
        self.enc, self.D, self.device, self.spec = enc, D, enc.device, spec
        self.op_mode = _operand_mode(enc.mode_name)
        self.weighted = bool(spec.use_weighted_layer_sum)
        check_xvector_head(head_sd, D, spec, L1)
        dims, n = tuple(int(d) for d in spec.tdnn_dim), len(spec.tdnn_dim)
        self.dim, self.n_out = int(spec.xvector_output_dim), int(head_sd["classifier.weight"].shape[0])
        if D % 64 or D > 2048:
            raise ValueError(f"XVectorHead needs a hidden width that is a multiple of 64 and at most 2048 (ser_gemm's K rule, ser_layer_mix_v's row), got {D}")
        if dims[-1] % 4:
            raise ValueError(f"tdnn_dim[-1] = {dims[-1]} is not a multiple of 4 (ser_stat_pool_v's 16-byte loads)")
        if not 1 <= self.dim <= _lib.CLS_TAIL_MAX or not 1 <= self.n_out <= _lib.CLS_TAIL_MAX:
            raise ValueError(f"xvector_output_dim {self.dim} / {self.n_out} labels: ser_xvec_tail_v takes 1..{_lib.CLS_TAIL_MAX} each")
        # padded widths: what a later GEMM reads as K chunks is a multiple of 64, the last layer's output a multiple of 8
        self.widths = [_pad_to(d, 64) for d in dims[:-1]] + [_pad_to(dims[-1], 8)]
        if max(self.widths[:-1], default=0) > 2048:
            raise ValueError(f"tdnn_dim {dims}: ser_act_rows_v takes rows of at most 2048 columns")
        f32 = lambda t: t.detach().to(torch.float32)                     # noqa: E731
        P0 = self.widths[0]
        w = torch.zeros((P0, D), dtype=torch.float32)
        b = torch.zeros(P0, dtype=torch.float32)
        w[: dims[0]], b[: dims[0]] = f32(head_sd["projector.weight"]), f32(head_sd["projector.bias"])
        self.projector = enc._linear(w, b, mode=self.op_mode, name="projector.weight")
        self.tdnn = []
        for i in range(n):
            k, d_in, p_in = int(spec.tdnn_kernel[i]), dims[i - 1] if i else dims[0], self.widths[i - 1] if i else P0
            w = torch.zeros((self.widths[i], k, p_in), dtype=torch.float32)
            b = torch.zeros(self.widths[i], dtype=torch.float32)
            w[: dims[i], :, :d_in] = f32(head_sd[f"tdnn.{i}.kernel.weight"]).reshape(dims[i], k, d_in)       # tap-major
            b[: dims[i]] = f32(head_sd[f"tdnn.{i}.kernel.bias"])
            self.tdnn.append(dict(lin=enc._linear(w.reshape(self.widths[i], k * p_in), b, mode=self.op_mode, name=f"tdnn.{i}.kernel.weight"),
                                  k=k, d=int(spec.tdnn_dilation[i]), p_in=p_in, N=self.widths[i]))
        self.Dl = dims[-1]
        self.F, self.bf = enc._dev_f32(head_sd["feature_extractor.weight"]), enc._dev_f32(head_sd["feature_extractor.bias"])
        self.C, self.bc = enc._dev_f32(head_sd["classifier.weight"]), enc._dev_f32(head_sd["classifier.bias"])
        # softmax(layer_weights), once, in float64 from the fp32 parameter
        sw = torch.softmax(head_sd["layer_weights"].detach().to(torch.float32).double(), dim=-1) if self.weighted else torch.ones(1, dtype=torch.float64)
        self.n_states = int(sw.numel())
        self.w = sw.contiguous().to(self.device)
        self._bufs = SlotArenas(self._build_buffers)

    def _build_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one pipeline slot, sized by the encoder rows M (every later level has fewer): the operand of the projector, one per
        TDNN layer's input, one fp32 GEMM output and one tap-0 row table that the layers take turns with (one stream), and the tail's"""
        M, B, dev = cap["M"], cap["B"], self.device
        planes, dt = _PLANES[self.op_mode], _DTYPE[self.op_mode]
        ops = [Act(M, self.D, planes, dev, dtype=dt)] + [Act(M, t["p_in"], planes, dev, dtype=dt) for t in self.tdnn]
        return dict(ops=ops, y=torch.empty((M, max(self.widths)), dtype=torch.float32, device=dev),
                    rowoff=torch.empty(M, dtype=torch.int32, device=dev),
                    work=torch.empty(cap["work"], dtype=torch.float64, device=dev),
                    stats=torch.empty((B, 2 * self.Dl), dtype=torch.float32, device=dev),
                    rows=torch.empty((B, self.dim + self.n_out), dtype=torch.float32, device=dev),      # [embeddings | logits]
                    # the encoder's frame offsets when they came without a device copy, then per layer its [B + 1] offsets and [B] base rows
                    tab=TableBlob(B, 1 + 2 * len(self.tdnn), dev))

    def forward(self, hs: HiddenStates, slot: int = 0):
        """(``[B, xvector_output_dim]`` fp32 embeddings, ``[B, num_labels]`` fp32 logits): the two column blocks of ``forward_rows``"""
        rows = self.forward_rows(hs, slot)
        return rows[:, : self.dim], rows[:, self.dim:]

    def forward_rows(self, hs: HiddenStates, slot: int = 0) -> torch.Tensor:
        """``[B, xvector_output_dim + num_labels]`` fp32 on the device, embeddings then logits (a view of the slot's buffer: valid until
        the slot's next ``forward``).  ``hs.states`` is only read.  ``ValueError`` naming the utterance (by index) whose TDNN output has
        fewer than two rows, before anything is launched."""
        if hs.computed < len(hs):
            raise IndexError(f"the head needs {'every hidden state' if self.weighted else 'the last hidden state'} (run the forward without "
                             f"last_state: states 0..{hs.computed - 1} of {len(hs)} were computed)")
        s = hs.states
        M, B, D = int(hs.frame_offs[-1]), hs.batch, self.D
        if s.dim() != 3 or s.shape[0] != self.enc.geo.num_layers + 1 or s.shape[2] != D or s.stride(2) != 1 or s.shape[1] < M \
                or s.dtype != torch.float32:
            raise ValueError(f"hidden states {tuple(s.shape)} do not match the head ({self.enc.geo.num_layers + 1} states of width {D}, {M} rows)")
        lay = self.spec.layout(hs.frame_offs)                             # refuses a short utterance by index
        offs = lay.offs
        max_out = max(offs[-1][b + 1] - offs[-1][b] for b in range(B))
        chunks = -(-max_out // _lib.STAT_POOL_FC)
        bf = self._bufs.fit(slot, M=M, B=B, work=B * chunks * 2 * self.Dl)
        st = _stream()
        tab = bf["tab"].begin()
        offs_dev = [hs.frame_offs_dev if hs.frame_offs_dev is not None else tab.put32(offs[0])]
        bases = []
        for i in range(len(self.tdnn)):
            offs_dev.append(tab.put32(offs[i + 1]))
            bases.append(tab.put64(offs[i][:B]))
        tab.send()
        flag = hs.range_flag.data_ptr() if (hs.range_flag is not None and self.op_mode == _lib.MODE_FP16X) else None
        ops, y, enc = bf["ops"], bf["y"], self.enc
        first = s if self.weighted else s[-1:]
        x0 = ops[0].first_rows(M)
        m = _lib.LayerMixArgs()
        m.s, m.state_stride, m.lds, m.w = first.data_ptr(), s.stride(0), s.stride(1), self.w.data_ptr()
        m.out_act, m.ldo_act, m.out_plane_stride, m.range_flag = x0.ptr, x0.cols, x0.plane_stride, flag
        m.n_states, m.mode, m.rows, m.D = self.n_states, self.op_mode, M, D
        self._step("layer_mix", lambda: check(lib.ser_layer_mix_v(C.byref(m), st), "ser_layer_mix_v"))
        prev_flag, prev_st = enc._flag, enc._st
        enc._flag, enc._st = flag, st                                     # the GEMMs' guard word and stream (launched at once, never recorded)
        try:
            self._step("projector", lambda: enc._gemm(x0, self.projector, M, out_act=ops[1].first_rows(M), mode=self.op_mode))
            for i, t in enumerate(self.tdnn):
                Mi, last = int(offs[i + 1][-1]), i == len(self.tdnn) - 1
                a_in, p_in, N = ops[i + 1].first_rows(int(offs[i][-1])), t["p_in"], t["N"]

                def layer(i=i, t=t, Mi=Mi, a_in=a_in, p_in=p_in, N=N):
                    check(lib.ser_ragged_index(offs_dev[i + 1].data_ptr(), bases[i].data_ptr(), B, 1, p_in, 8, bf["rowoff"].data_ptr(), Mi, st),
                          "ser_ragged_index")
                    enc._gemm(a_in, t["lin"], Mi, a_rowoff=bf["rowoff"], kc=p_in, ldj=t["d"] * p_in, out_f32=y, ldo_f32=N, mode=self.op_mode)
                self._step(f"tdnn{i}", layer)
                if not last:
                    nxt = ops[i + 2].first_rows(Mi)
                    r = _lib.ActRowsArgs()
                    r.x, r.ldx, r.out_act, r.ldo_act, r.out_plane_stride = y.data_ptr(), N, nxt.ptr, nxt.cols, nxt.plane_stride
                    r.range_flag, r.relu, r.mode, r.rows, r.D = flag, 1, self.op_mode, Mi, N
                    self._step(f"relu{i}", lambda r=r: check(lib.ser_act_rows_v(C.byref(r), st), "ser_act_rows_v"))
        finally:
            enc._flag, enc._st = prev_flag, prev_st
        Ml, Nl = int(offs[-1][-1]), self.widths[-1]
        offs_host = (C.c_int32 * (B + 1))(*offs[-1])
        p = _lib.StatPoolArgs()
        p.x, p.ldx, p.frame_offs, p.frame_offs_host = y.data_ptr(), Nl, offs_dev[-1].data_ptr(), C.cast(offs_host, C.c_void_p)
        p.work, p.work_elems, p.out, p.ldo = bf["work"].data_ptr(), bf["work"].numel(), bf["stats"].data_ptr(), 2 * self.Dl
        p.B, p.D, p.rows, p.max_frames, p.relu = B, self.Dl, Ml, max_out, 1
        self._step("stat_pool", lambda: check(lib.ser_stat_pool_v(C.byref(p), st), "ser_stat_pool_v"))
        t = _lib.XvecTailArgs()
        t.stats, t.lds, t.F, t.bf, t.C, t.bc = bf["stats"].data_ptr(), 2 * self.Dl, self.F.data_ptr(), self.bf.data_ptr(), self.C.data_ptr(), self.bc.data_ptr()
        ld = self.dim + self.n_out
        t.emb, t.lde, t.logits, t.ldo = bf["rows"].data_ptr(), ld, bf["rows"].data_ptr() + 4 * self.dim, ld
        t.B, t.D, t.dim, t.n_labels = B, 2 * self.Dl, self.dim, self.n_out
        self._step("xvec_tail", lambda: check(lib.ser_xvec_tail_v(C.byref(t), st), "ser_xvec_tail_v"))
        return bf["rows"][:B]


class CTCHead(_HeadBase):
    """The head of the hub's CTC checkpoints on the device (HF Wav2Vec2ForCTC.forward and its HuBERT / WavLM / data2vec-audio / w2v-BERT
    twins, then ``argmax(-1)`` and what ``Wav2Vec2CTCTokenizer`` does to the ids): ``last_hidden_state`` -> lm_head -> per frame the
    winning id -> equal neighbours merged, blanks dropped.  ``forward_tokens`` enqueues three steps on the current stream behind the
    encoder's recorded forward (no command-list op, the tapes stay as they are):
      ser_layer_mix_v (one state, weight 1: the identity in fp32, the last state as the GEMM's operand planes)
      -> ser_gemm (lm_head, fp32 out; ``lm_head.weight`` zero-padded at load to a multiple of 8 rows)
      -> ser_ctc_greedy_v with the TRUE vocabulary width: it never reads the padded columns, so their zeros cannot win.
    Every utterance alone: the collapse compares a frame with the previous frame of its own utterance only, and nothing is summed.  GEMM
    operand format: bf16 in mode "bf16", bf16 hi + lo in "fp32x", fp16 hi + lo otherwise; the fp16 copies report to ``hs.range_flag``.
    ``head_sd``: the tensors of ``weights.split_ctc_head``; ``spec``: ``config.CTCSpec``."""

    def __init__(self, enc: "_EncoderBase", head_sd, spec):
        from .weights import check_ctc_head
        if not isinstance(enc, (SpeechEncoder, W2vBertEncoder)):
            raise ValueError("CTCHead runs behind the speech and w2v-BERT encoders")
        D = enc.geo.hidden
        self.enc, self.D, self.device, self.spec = enc, D, enc.device, spec
        self.op_mode = _operand_mode(enc.mode_name)
        self.V, self.blank = int(spec.vocab_size), int(spec.blank)
        if D % 64 or D > 2048:
            raise ValueError(f"CTCHead needs a hidden width that is a multiple of 64 and at most 2048 (ser_gemm's K rule, ser_layer_mix_v's row), got {D}")
        check_ctc_head(head_sd, D, self.V)
        self.Vp = _pad_to(self.V, 8)
        w = torch.zeros((self.Vp, D), dtype=torch.float32)
        b = torch.zeros(self.Vp, dtype=torch.float32)
        w[: self.V], b[: self.V] = head_sd["lm_head.weight"].detach().to(torch.float32), head_sd["lm_head.bias"].detach().to(torch.float32)
        self.lm_head = enc._linear(w, b, mode=self.op_mode, name="lm_head.weight")
        self.w = torch.ones(1, dtype=torch.float64, device=self.device)
        self._bufs = SlotArenas(self._build_buffers)
        self._abufs = SlotArenas(self._build_align_buffers)
        self._last: Dict[int, tuple] = {}                                 # slot -> (M, B, max_frames) of its last forward

    @staticmethod
    def blob_words(B: int, max_frames: int) -> int:
        """int32 words of a batch's result: counts [B] | ids [B, Tm] | starts [B, Tm] | ends [B, Tm] | min_margin [B] (fp32 bits) | err [1]"""
        return 2 * B + 3 * B * max_frames + 1

    @staticmethod
    def unpack(words, B: int, max_frames: int) -> dict:
        """The host copy of ``forward_tokens``'s buffer (numpy int32 [blob_words]) as its parts (views)"""
        import numpy as np
        w = np.asarray(words).reshape(-1).view(np.int32)
        n = B * max_frames
        part = lambda i: w[B + i * n: B + (i + 1) * n].reshape(B, max_frames)      # noqa: E731
        return dict(counts=w[:B], ids=part(0), starts=part(1), ends=part(2), min_margin=w[B + 3 * n: 2 * B + 3 * n].view(np.float32),
                    err=int(w[2 * B + 3 * n]))

    def _build_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one pipeline slot: the operand copy of the last state, the fp32 logits, the kernel's per-frame words, the result"""
        M, dev = cap["M"], self.device
        return dict(xa=Act(M, self.D, _PLANES[self.op_mode], dev, dtype=_DTYPE[self.op_mode]),
                    z=torch.empty((M, self.Vp), dtype=torch.float32, device=dev),
                    work=torch.empty(2 * M, dtype=torch.int32, device=dev),
                    blob=torch.empty(cap["blob"], dtype=torch.int32, device=dev), tab=TableBlob(cap["B"], 1, dev))

    def _lm_head(self, hs: HiddenStates, slot: int, blob: Callable[[int, int], int]):
        """The part ``forward_tokens`` and ``forward_align`` share: the operand copy of the last state and the lm_head GEMM into the slot's
        fp32 logits.  Returns (the slot's buffers, the device frame offsets, rows, B, the longest utterance's frames, the stream);
        ``blob(B, frames)``: the words the caller needs of the slot's token blob."""
        if hs.computed < len(hs):
            raise IndexError(f"the head needs the last hidden state (run the forward without last_state: states 0..{hs.computed - 1} of "
                             f"{len(hs)} were computed)")
        s = hs.states
        M, B, D = int(hs.frame_offs[-1]), hs.batch, self.D
        if s.dim() != 3 or s.shape[2] != D or s.stride(2) != 1 or s.shape[1] < M or s.dtype != torch.float32:
            raise ValueError(f"hidden states {tuple(s.shape)} do not match the head (states of width {D}, {M} rows)")
        Tm = max(hs.frames(b) for b in range(B))
        if M < 1 or Tm < 1:
            raise ValueError("the batch has no frames")
        bf = self._bufs.fit(slot, M=M, B=B, blob=blob(B, Tm))
        st = _stream()
        offs = hs.frame_offs_dev if hs.frame_offs_dev is not None else _head_offs(bf["tab"], hs.frame_offs)
        flag = hs.range_flag.data_ptr() if (hs.range_flag is not None and self.op_mode == _lib.MODE_FP16X) else None
        enc, xa, z = self.enc, bf["xa"].first_rows(M), bf["z"]
        m = _lib.LayerMixArgs()
        m.s, m.state_stride, m.lds, m.w = s[-1].data_ptr(), 0, s.stride(1), self.w.data_ptr()
        m.out_act, m.ldo_act, m.out_plane_stride, m.range_flag = xa.ptr, xa.cols, xa.plane_stride, flag
        m.n_states, m.mode, m.rows, m.D = 1, self.op_mode, M, D
        self._step("operand", lambda: check(lib.ser_layer_mix_v(C.byref(m), st), "ser_layer_mix_v"))
        prev_flag, prev_st = enc._flag, enc._st
        enc._flag, enc._st = flag, st                                     # the GEMM's guard word and stream (launched at once, never recorded)
        try:
            self._step("lm_head", lambda: enc._gemm(xa, self.lm_head, M, out_f32=z, ldo_f32=self.Vp, mode=self.op_mode))
        finally:
            enc._flag, enc._st = prev_flag, prev_st
        self._last[slot] = (M, B, Tm)
        return bf, offs, M, B, Tm, st

    def forward_tokens(self, hs: HiddenStates, slot: int = 0) -> torch.Tensor:
        """int32 [blob_words(B, max_frames)] on the device (``unpack`` names its parts; a view of the slot's buffer, valid until the slot's
        next forward): one D2H copy brings a batch's counts, ids, offsets, smallest margins and error word back.  ``hs.states`` is only read."""
        bf, offs, M, B, Tm, st = self._lm_head(hs, slot, self.blob_words)
        n = self.blob_words(B, Tm)
        z, blob = bf["z"], bf["blob"]
        blob[n - 1: n].zero_()                                            # the error word
        p0, nt = blob.data_ptr(), 4 * B * Tm
        g = _lib.CtcGreedyArgs()
        g.z, g.ldz, g.frame_offs, g.work, g.work_elems = z.data_ptr(), self.Vp, offs.data_ptr(), bf["work"].data_ptr(), bf["work"].numel()
        g.counts, g.ids, g.starts, g.ends, g.ld_tok = p0, p0 + 4 * B, p0 + 4 * B + nt, p0 + 4 * B + 2 * nt, Tm
        g.min_margin, g.err = p0 + 4 * B + 3 * nt, p0 + 4 * (n - 1)
        g.B, g.V, g.rows, g.blank, g.max_frames = B, self.V, M, self.blank, Tm
        self._step("ctc_greedy", lambda: check(lib.ser_ctc_greedy_v(C.byref(g), st), "ser_ctc_greedy_v"))
        return blob[:n]

    # ---- forced alignment (ser_ctc_align_v): the same logits, a given target per utterance
    @staticmethod
    def align_words(B: int, max_tokens: int, rows: int = 0) -> int:
        """int32 words of a batch's alignment: status [B] | starts [B, Lm] | ends [B, Lm] | tok_score [B, Lm] (fp32 bits) | one pad word
        when that many are odd | path_logit [B] (float64 bits, two words each) | with ``rows``: pos [rows] | frame_score [rows] (fp32 bits);
        Lm = max(max_tokens, 1)"""
        return CTCHead._align_tail(B, max(int(max_tokens), 1)) + 2 * B + 2 * rows

    @staticmethod
    def _align_tail(B: int, Lm: int) -> int:
        """the word offset of path_logit: behind status and the three [B, Lm] tables, rounded up to an even word (8-byte aligned)"""
        n = B + 3 * B * Lm
        return n + (n & 1)

    @staticmethod
    def unpack_align(words, B: int, max_tokens: int, rows: int = 0) -> dict:
        """The host copy of ``forward_align``'s buffer (numpy int32 [align_words]) as its parts (views)"""
        import numpy as np
        w = np.asarray(words).reshape(-1).view(np.int32)
        Lm = max(int(max_tokens), 1)
        n = B * Lm
        part = lambda i: w[B + i * n: B + (i + 1) * n].reshape(B, Lm)             # noqa: E731
        o = CTCHead._align_tail(B, Lm)
        out = dict(status=w[:B], starts=part(0), ends=part(1), tok_score=part(2).view(np.float32), path_logit=w[o: o + 2 * B].view(np.float64))
        if rows:
            out["pos"] = w[o + 2 * B: o + 2 * B + rows]
            out["frame_score"] = w[o + 2 * B + rows: o + 2 * B + 2 * rows].view(np.float32)
        return out

    def _build_align_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one slot's alignment: the kernel's work bytes, the result, and the blob that carries tgt_offs | targets up (one
        region each: ``tab`` regions hold 2 cap + 4 int32 words)"""
        dev = self.device
        return dict(work=torch.empty((cap["work"] + 7) // 8, dtype=torch.int64, device=dev),
                    blob=torch.empty(cap["blob"], dtype=torch.int32, device=dev), tab=TableBlob(cap["tab"], 2, dev))

    def forward_align(self, hs: HiddenStates, targets, slot: int = 0, frames: bool = False) -> torch.Tensor:
        """int32 [align_words(B, max tokens, rows if frames)] on the device (``unpack_align`` names its parts; a view of the slot's
        buffer, valid until the slot's next ``forward_align``): the best CTC path of utterance b that spells ``targets[b]`` (a sequence
        of token ids), behind the same operand copy and lm_head as ``forward_tokens``.  A target the kernel refuses (an id outside the
        vocabulary, the blank, more than ``_lib.CTC_ALIGN_MAX_TOKENS`` ids) or cannot place comes back in that utterance's status word."""
        B = hs.batch
        if len(targets) != B:
            raise ValueError(f"{len(targets)} targets for a batch of {B}")
        tgt_offs = [0]
        for y in targets:
            tgt_offs.append(tgt_offs[-1] + len(y))
        flat = [int(v) for y in targets for v in y]
        nt = len(flat)
        Lm = min(max(len(y) for y in targets), _lib.CTC_ALIGN_MAX_TOKENS)          # a longer target is the kernel's BAD_TARGET
        bf, offs, M, B, Tm, st = self._lm_head(hs, slot, lambda B, Tm: 1)        # (the token blob is forward_tokens')
        n = self.align_words(B, Lm, M if frames else 0)
        wb = int(lib.ser_ctc_align_work_bytes(M, B, Tm, Lm))
        ab = self._abufs.fit(slot, work=wb, blob=n, tab=max(B, (nt + 1) // 2))
        tab = ab["tab"].begin()
        d_offs, d_tgt = tab.put32(tgt_offs), tab.put32(flat or [0])       # (never an empty view: its address is an argument)
        tab.send()
        blob, Lp = ab["blob"], max(Lm, 1)
        p0, o = blob.data_ptr(), self._align_tail(B, Lp)
        a = _lib.CtcAlignArgs()
        a.z, a.ldz, a.frame_offs, a.targets, a.tgt_offs = bf["z"].data_ptr(), self.Vp, offs.data_ptr(), d_tgt.data_ptr(), d_offs.data_ptr()
        a.work, a.work_bytes = ab["work"].data_ptr(), 8 * ab["work"].numel()
        a.status, a.starts, a.ends, a.tok_score, a.ld_tok = p0, p0 + 4 * B, p0 + 4 * (B + B * Lp), p0 + 4 * (B + 2 * B * Lp), Lp
        a.path_logit = p0 + 4 * o
        a.pos, a.frame_score = (p0 + 4 * (o + 2 * B), p0 + 4 * (o + 2 * B + M)) if frames else (None, None)
        a.B, a.V, a.rows, a.blank, a.max_frames, a.max_tokens, a.n_targets = B, self.V, M, self.blank, Tm, Lm, nt
        self._step("ctc_align", lambda: check(lib.ser_ctc_align_v(C.byref(a), st), "ser_ctc_align_v"))
        return blob[:n]

    def logits(self, slot: int = 0) -> torch.Tensor:
        """fp32 [rows, vocab_size] logits of the slot's last forward (a view of its buffer), for tests and tools"""
        return self._bufs[slot]["z"][: self._last[slot][0], : self.V]

    def status(self, slot: int = 0) -> int:
        """the error word of the slot's last forward (synchronous): ``_lib.CTC_ERR_NONFINITE`` when a frame's winning logit was not finite"""
        M, B, Tm = self._last[slot]
        return int(self._bufs[slot]["blob"][self.blob_words(B, Tm) - 1].item())


def _fusion_keys(names) -> Dict[str, tuple]:
    """state-dict keys and symbolic shapes of the reference's fusion head over the modalities ``names`` (feature width of modality i: "d<i+1>")"""
    keys = {"classifier.0.weight": ("h1", "ne"), "classifier.0.bias": ("h1",), "classifier.3.weight": ("n", "h1"), "classifier.3.bias": ("n",),
            "layer_norm.weight": ("ne",), "layer_norm.bias": ("ne",)}
    for i, m in enumerate(names):
        keys.update({f"{m}_projection.weight": ("h", f"d{i + 1}"), f"{m}_projection.bias": ("h",), f"{m}_norm.weight": ("h",),
                     f"{m}_norm.bias": ("h",), f"{m}_attn.weight": (1, "e"), f"{m}_attn.bias": (1,),
                     f"{m}_attention.in_proj_weight": ("3e", "e"), f"{m}_attention.in_proj_bias": ("3e",),
                     f"{m}_attention.out_proj.weight": ("e", "e"), f"{m}_attention.out_proj.bias": ("e",)})
        for sfx in ("", "_reverse"):
            keys.update({f"{m}_gru.weight_ih_l0{sfx}": ("3h", "h"), f"{m}_gru.weight_hh_l0{sfx}": ("3h", "h"),
                         f"{m}_gru.bias_ih_l0{sfx}": ("3h",), f"{m}_gru.bias_hh_l0{sfx}": ("3h",)})
    return keys


FUSION_KEYS = _fusion_keys(("speech", "text"))
TRIMODAL_KEYS = _fusion_keys(("speech", "text", "prosody"))
FUSION_BATCH = 16                                                 # utterances per MFMA column group of ser_gru_v


class RowSource:
    """Rows a device head reads where they lie, in place of a packed ``[M, D]`` tensor: utterance b's row t is row ``src_offs[b] + t`` of
    ``states`` -- one fp32 ``[rows, D]`` device view, or four of equal pitch for the mean of the four (``mean_last4``'s value, no buffer of
    its own).  The counts are the head's packed offsets; ``src_offs`` need not ascend, and rows no utterance selects (a Whisper window
    behind its crop) are never read."""

    def __init__(self, states, src_offs: Sequence[int]):
        self.states = [states] if isinstance(states, torch.Tensor) else list(states)
        self.src_offs = [int(v) for v in src_offs]

    def check(self, what: str, offs: Sequence[int], D: int, device) -> None:
        st = self.states
        if len(st) not in (1, 4):
            raise ValueError(f"{what} rows: a RowSource holds one state, or four for their mean, got {len(st)}")
        for x in st:
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != D or x.stride(1) != 1 \
                    or x.stride(0) % 4 or x.stride(0) < D or x.data_ptr() % 16 or x.device != device:
                raise ValueError(f"{what} rows must be fp32 [rows, {D}] views on {device} (16-byte aligned, row pitch a multiple of 4)")
        if any(x.stride(0) != st[0].stride(0) for x in st):
            raise ValueError(f"{what} rows: the four states of a mean must share one row pitch")
        B, rows = len(offs) - 1, min(int(x.shape[0]) for x in st)
        if len(self.src_offs) != B:
            raise ValueError(f"{what} rows: {len(self.src_offs)} source offsets for {B} utterances")
        for b, s0 in enumerate(self.src_offs):
            if s0 < 0 or s0 + (offs[b + 1] - offs[b]) > rows:
                raise ValueError(f"{what} rows: utterance {b} selects rows {s0} .. {s0 + offs[b + 1] - offs[b] - 1} of a {rows}-row source")


class _FusionBase(_HeadBase):
    """The reference's fusion heads over the modalities ``NAMES`` (the prefixes of their state-dict keys), on packed ragged batches, EVERY
    UTTERANCE ALONE.  Everything of one ``forward`` goes on the current stream, in order: a ser_gru_v cluster makes progress only while all
    of its blocks are resident, so two recurrences are never in flight together.  Per modality
      ser_pack_rows_flagged -> ser_gemm (projection) -> ser_layernorm_v (operand copy) -> ser_gemm (both directions' x W_ih^T) -> ser_gru_v
    then one q GEMM per attention module (queries: the module's own modality), one k | v GEMM per modality (its GRU output under the k | v
    rows of every OTHER module's in_proj_weight, stacked), one cross-attention and one out-projection per (module, other modality) -- a
    module's second out-projection adds its first through ser_gemm's residual epilogue --, one ser_attn_pool_v per modality and
    ser_fusion_cls_v on the [B, n E] row.  A modality handed in as a ``RowSource`` replaces its ser_pack_rows_flagged by one ser_select_rows_v
    into the same operand copy (same range-guard word, same place in the order); everything behind it is untouched."""
    NAMES: tuple = ()
    KEYS: Dict[str, tuple] = {}
    WHAT = "fusion head"

    def _init(self, state_dict, dims_in: Sequence[int], heads: Sequence[int], device, mode: str, cluster: int) -> None:
        names, n = self.NAMES, len(self.NAMES)
        if mode not in MODES:
            raise ValueError(f"mode must be one of {list(MODES)}")
        self.op_mode = _operand_mode(mode)
        if any(d <= 0 or d % 64 for d in dims_in):
            raise ValueError(f"{type(self).__name__} needs feature widths that are multiples of 64 (ser_gemm's K rule), got "
                             + " ".join(f"D{i + 1}={d}" for i, d in enumerate(dims_in)))
        sd = state_dict
        missing = [k for k in self.KEYS if k not in sd]                # keys beyond the head's own (a ranking checkpoint's second classifier) are ignored
        if missing:
            raise ValueError(f"the head's state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''} ({len(missing)} keys)")
        h = int(sd["speech_norm.weight"].shape[0])
        if h % 64 or not 64 <= h <= 512:
            raise ValueError(f"fusion hidden width {h}: ser_gru_v runs multiples of 64 up to 512")
        h1, n_out = int(sd["classifier.0.weight"].shape[0]), int(sd["classifier.3.weight"].shape[0])
        if not 1 <= n_out <= 8:
            raise ValueError(f"classifier.3.weight has {n_out} outputs (1..8)")
        E = 2 * h
        heads = tuple(int(v) for v in heads)
        if len(heads) != n or any(v < 1 or E % v or (E // v) % 64 for v in heads):
            raise ValueError(f"heads={heads}: one count per attention module ({', '.join(names)}), each dividing E = {E} into multiples of 64")
        dims = {"h": h, "3h": 3 * h, "e": E, "ne": n * E, "3e": 3 * E, "h1": h1, "n": n_out}
        dims.update({f"d{i + 1}": d for i, d in enumerate(dims_in)})
        for k, want in self.KEYS.items():
            want = tuple(dims.get(w, w) for w in want)
            if tuple(sd[k].shape) != want:
                raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, expected {want}")
        self.host = host = _LaunchHost(device, mode, self.op_mode, self.op_mode, self.op_mode == _lib.MODE_FP16X)
        self.device, self.mode_name = host.device, mode
        self.h, self.E, self.h1, self.n_out, self.dims_in, self.heads, self.cluster = h, E, h1, n_out, tuple(dims_in), heads, int(cluster)
        om = self.op_mode
        f32 = host._dev_f32
        self.mod = []
        for name in names:
            gru = f"{name}_gru"
            wih = torch.cat([sd[f"{gru}.weight_ih_l0"], sd[f"{gru}.weight_ih_l0_reverse"]], dim=0)
            whh = torch.cat([sd[f"{gru}.weight_hh_l0"], sd[f"{gru}.weight_hh_l0_reverse"]], dim=0)
            self.mod.append(dict(
                proj=host._linear(sd[f"{name}_projection.weight"], sd[f"{name}_projection.bias"], mode=om, name=f"{name}_projection.weight"),
                ln=(f32(sd[f"{name}_norm.weight"]), f32(sd[f"{name}_norm.bias"])),
                wih=host._linear(wih, torch.cat([sd[f"{gru}.bias_ih_l0"], sd[f"{gru}.bias_ih_l0_reverse"]]), mode=om, name=f"{gru}.weight_ih_l0"),
                # the recurrent weights: fp16 hi + lo planes in every mode; an element beyond fp16's range is refused here, by name
                whh=host._linear(whh, None, mode=_lib.MODE_FP16X, name=f"{gru}.weight_hh_l0"),
                bhh=f32(torch.cat([sd[f"{gru}.bias_hh_l0"], sd[f"{gru}.bias_hh_l0_reverse"]]))))
        self.others = [[j for j in range(n) if j != i] for i in range(n)]
        self.att = []
        for name in names:                                        # attention module whose queries are this modality's rows
            w, b = sd[f"{name}_attention.in_proj_weight"], sd[f"{name}_attention.in_proj_bias"]
            self.att.append(dict(
                q=host._linear(w[:E], b[:E], mode=om, name=f"{name}_attention.in_proj_weight"),
                out=host._linear(sd[f"{name}_attention.out_proj.weight"], sd[f"{name}_attention.out_proj.bias"], mode=om,
                                 name=f"{name}_attention.out_proj.weight"),
                pool_w=f32(sd[f"{name}_attn.weight"].reshape(E)), pool_b=float(sd[f"{name}_attn.bias"].reshape(-1)[0])))
        for j, name in enumerate(names):                          # modality j's rows under the k | v rows of every other module, stacked
            ws = [sd[f"{names[i]}_attention.in_proj_weight"][E:] for i in self.others[j]]
            bs = [sd[f"{names[i]}_attention.in_proj_bias"][E:] for i in self.others[j]]
            self.mod[j]["kv"] = host._linear(torch.cat(ws, dim=0), torch.cat(bs), mode=om,
                                             name=" | ".join(f"{names[i]}_attention.in_proj_weight" for i in self.others[j]))
        self.ln_g, self.ln_b = f32(sd["layer_norm.weight"]), f32(sd["layer_norm.bias"])
        self.w1, self.b1 = f32(sd["classifier.0.weight"]), f32(sd["classifier.0.bias"])
        self.w2, self.b2 = f32(sd["classifier.3.weight"]), f32(sd["classifier.3.bias"])
        r = C.c_int32(0)
        self.work_bytes = int(lib.ser_gru_work_bytes(h, self.cluster, C.byref(r)))
        if self.work_bytes < 0:
            raise ValueError(f"cluster={cluster} does not divide H / 16 = {h // 16}")
        self.R = r.value
        self._epoch = 1
        self._bufs = SlotArenas(self._build_buffers)

    def _build_buffers(self, cap: Dict[str, int]) -> dict:
        """buffers of one pipeline slot; ``cap``: utterances B and the rows M1, M2 (, M3) of each side"""
        dev, h, E, om, n = self.device, self.h, self.E, self.op_mode, len(self.NAMES)
        B, Ms = cap["B"], [cap[f"M{i + 1}"] for i in range(n)]
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        act = lambda rows, cols: Act(rows, cols, _PLANES[om], dev, dtype=_DTYPE[om])
        side = []
        for M, D in zip(Ms, self.dims_in):
            sb = dict(xa=act(M, D), proj=f(M, h), sa=act(M, h), gx=f(M, 6 * h), gh=f(M, E), gha=act(M, E), q=f(M, E), kv=f(M, 2 * E * (n - 1)),
                      ctx=[act(M, E) for _ in range(n - 1)], att=f(M, E), scores=f(M))
            if n > 2:
                sb["att_first"] = f(M, E)                         # the first out-projection of a module with two key sides (distinct from `att`)
            side.append(sb)
        return dict(side=side, tab=TableBlob(B, 2 * n, dev), pooled=f(B, n * E), xn=f(B, n * E), hidden=f(B, self.h1), out=f(B, self.n_out),
                    err=torch.zeros(1, dtype=torch.int32, device=dev), flag=torch.zeros(1, dtype=torch.int32, device=dev),
                    work=torch.zeros(max(self.work_bytes, 16), dtype=torch.uint8, device=dev))

    def _gru(self, bf, sb, w, B: int, M: int, max_frames: int, st: int) -> None:
        g = _lib.GruArgs()
        g.gx, g.ldgx, g.whh, g.whh_plane_stride, g.bhh = sb["gx"].data_ptr(), 6 * self.h, w["whh"].w.data_ptr(), 6 * self.h * self.h, w["bhh"].data_ptr()
        g.frame_offs, g.out, g.ldo = sb["offs"].data_ptr(), sb["gh"].data_ptr(), self.E
        g.out_act, g.ldo_act, g.out_plane_stride = sb["gha"].ptr, self.E, sb["gha"].plane_stride
        g.work, g.work_bytes, g.err = bf["work"].data_ptr(), self.work_bytes, bf["err"].data_ptr()
        g.B, g.H, g.rows, g.max_frames, g.mode, g.cluster, g.epoch = B, self.h, M, max_frames, self.op_mode, self.cluster, self._epoch & 0xFFFFFFFF
        self._epoch += 1 + B // FUSION_BATCH
        check(lib.ser_gru_v(C.byref(g), st), "ser_gru_v")

    def _forward(self, xs: Sequence[torch.Tensor], offs_in: Sequence[Sequence[int]], slot: int, range_flag: Optional[torch.Tensor]) -> torch.Tensor:
        names, n = self.NAMES, len(self.NAMES)
        offs = [[int(v) for v in o] for o in offs_in]
        B = len(offs[0]) - 1
        if B < 1 or any(len(o) != B + 1 for o in offs):
            raise ValueError(" and ".join(f"offs{i + 1}" for i in range(n)) + " must list the same number (>= 1) of utterances")
        Ms, host, E, h, om = [o[-1] for o in offs], self.host, self.E, self.h, self.op_mode
        for i, (x, D, what) in enumerate(zip(xs, self.dims_in, names)):
            if offs[i][0] != 0 or any(b <= a for a, b in zip(offs[i][:-1], offs[i][1:])):
                raise ValueError(f"an empty {what} utterance (or offsets that do not ascend from 0): every utterance needs at least one row")
            if isinstance(x, RowSource):
                x.check(what, offs[i], D, self.device)
                continue
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != D or x.shape[0] < Ms[i] or x.stride(1) != 1 or x.stride(0) % 4 \
                    or x.data_ptr() % 16 or x.device != self.device:
                raise ValueError(f"{what} rows must be an fp32 [>= {Ms[i]}, {D}] tensor on {self.device} (16-byte aligned, row pitch a multiple of 4)")
        bf = self._bufs.fit(slot, B=B, **{f"M{i + 1}": M for i, M in enumerate(Ms)})
        st = _stream()
        flag_t = range_flag if range_flag is not None else bf["flag"]
        bf["flag_used"] = flag_t
        flag = flag_t.data_ptr() if om == _lib.MODE_FP16X else None
        host._flag = flag
        bf["err"].zero_()
        maxf = [max(b - a for a, b in zip(o[:-1], o[1:])) for o in offs]
        tab = bf["tab"].begin()
        for sb, o, x in zip(bf["side"], offs, xs):                # per side: its offsets, and its source rows where it is a RowSource
            sb["offs"], sb["src"] = tab.put32(o), tab.put32(x.src_offs if isinstance(x, RowSource) else ())
        tab.send()
        for i in range(n):
            sb, w, x, M = bf["side"][i], self.mod[i], xs[i], Ms[i]
            D = self.dims_in[i]
            xa, sa = sb["xa"].first_rows(M), sb["sa"].first_rows(M)
            tag = names[i]
            if isinstance(x, RowSource):                          # the utterances' rows where they lie: one ragged gather into the same operand copy
                g = _lib.SelectRowsArgs()
                for k, s_ in enumerate(x.states):
                    g.src[k] = s_.data_ptr()
                g.ld_src, g.src_offs, g.dst_offs = x.states[0].stride(0), sb["src"].data_ptr(), sb["offs"].data_ptr()
                g.out_act, g.ldo_act, g.out_plane_stride, g.range_flag = xa.ptr, D, xa.plane_stride, flag
                g.n_src, g.B, g.D, g.max_rows, g.mode = len(x.states), B, D, maxf[i], om
                self._step(f"{tag} pack", lambda: check(lib.ser_select_rows_v(C.byref(g), st), "ser_select_rows_v"))
            else:
                self._step(f"{tag} pack", lambda: check(lib.ser_pack_rows_flagged(x.data_ptr(), x.stride(0), 1, M, D, 0, xa.ptr, D, xa.plane_stride, om,
                                                                                 flag, st), "ser_pack_rows_flagged"))
            self._step(f"{tag} projection", lambda: host._gemm(xa, w["proj"], M, out_f32=sb["proj"], ldo_f32=h, mode=om))
            self._step(f"{tag} layernorm", lambda: host._layernorm(sb["proj"], h, w["ln"], M, h, out_act=sa, eps=1e-5))
            self._step(f"{tag} gx", lambda: host._gemm(sa, w["wih"], M, out_f32=sb["gx"], ldo_f32=6 * h, mode=om))
            self._step(f"{tag} gru", lambda: self._gru(bf, sb, w, B, M, maxf[i], st))
        ldkv = 2 * E * (n - 1)
        for i in range(n):                                        # q: module i over its own modality; k | v: modality i under every other module
            sb = bf["side"][i]
            gha = sb["gha"].first_rows(Ms[i])
            self._step(f"{names[i]} q", lambda: host._gemm(gha, self.att[i]["q"], Ms[i], out_f32=sb["q"], ldo_f32=E, mode=om))
            self._step(f"{names[i]} kv", lambda: host._gemm(gha, self.mod[i]["kv"], Ms[i], out_f32=sb["kv"], ldo_f32=ldkv, mode=om))
        for i in range(n):                                        # attention module i: queries of side i, keys / values of each other side
            sq = bf["side"][i]
            for t, j in enumerate(self.others[i]):
                sk = bf["side"][j]
                kcol = 2 * E * self.others[j].index(i)            # module i's k | v block inside modality j's stacked projection
                ctx = sq["ctx"][t].first_rows(Ms[i])
                xa = _lib.XattnMhArgs()
                xa.q, xa.ldq, xa.k, xa.ldk = sq["q"].data_ptr(), E, sk["kv"].data_ptr() + 4 * kcol, ldkv
                xa.v, xa.ldv = sk["kv"].data_ptr() + 4 * (kcol + E), ldkv
                xa.q_offs, xa.k_offs = sq["offs"].data_ptr(), sk["offs"].data_ptr()
                xa.out_act, xa.ldo_act, xa.out_plane_stride, xa.range_flag = ctx.ptr, E, ctx.plane_stride, flag
                xa.scale, xa.B, xa.E, xa.q_rows, xa.k_rows, xa.max_q, xa.mode = float(E // self.heads[i]) ** -0.5, B, E, Ms[i], Ms[j], maxf[i], om
                xa.heads = self.heads[i]
                self._step(f"{names[i]} xattn" + (f" {names[j]}" if n > 2 else ""), lambda: check(lib.ser_xattn_mh_v(C.byref(xa), st), "ser_xattn_mh_v"))
        for i in range(n):
            sq, a = bf["side"][i], self.att[i]
            for t, j in enumerate(self.others[i]):
                last = t == n - 2
                self._step(f"{names[i]} out_proj" + (f" {names[j]}" if n > 2 else ""),
                           lambda: host._gemm(sq["ctx"][t].first_rows(Ms[i]), a["out"], Ms[i], out_f32=sq["att"] if last else sq["att_first"], ldo_f32=E,
                                              residual=sq["att_first"] if (last and t > 0) else None, ldr=E if (last and t > 0) else 0, mode=om))
        for i in range(n):
            sq, a = bf["side"][i], self.att[i]
            p = _lib.AttnPoolArgs()
            p.a, p.lda, p.b, p.ldb, p.w, p.frame_offs = sq["gh"].data_ptr(), E, sq["att"].data_ptr(), E, a["pool_w"].data_ptr(), sq["offs"].data_ptr()
            p.scores, p.out, p.ldo, p.bias, p.col0 = sq["scores"].data_ptr(), bf["pooled"].data_ptr(), n * E, a["pool_b"], i * E
            p.B, p.E, p.rows, p.max_frames = B, E, Ms[i], maxf[i]
            self._step(f"{names[i]} attn_pool", lambda: check(lib.ser_attn_pool_v(C.byref(p), st), "ser_attn_pool_v"))
        c = _lib.FusionClsArgs()
        c.p, c.ldp, c.gamma, c.beta = bf["pooled"].data_ptr(), n * E, self.ln_g.data_ptr(), self.ln_b.data_ptr()
        c.W1, c.b1, c.W2, c.b2 = self.w1.data_ptr(), self.b1.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr()
        c.xn, c.hidden, c.out, c.eps = bf["xn"].data_ptr(), bf["hidden"].data_ptr(), bf["out"].data_ptr(), 1e-5
        c.B, c.K, c.H1, c.n_out = B, n * E, self.h1, self.n_out
        self._step("classifier", lambda: check(lib.ser_fusion_cls_v(C.byref(c), st), "ser_fusion_cls_v"))
        host._flag = None
        return bf["out"][:B]

    def status(self, slot: int = 0):
        """(range-guard bits, ser_gru_v error word) of the slot's last ``forward``, read back (synchronises); both words are cleared."""
        bf = self._bufs[slot]
        flag_t = bf.get("flag_used", bf["flag"])
        bits, err = int(flag_t.item()), int(bf["err"].item())
        flag_t.zero_()
        return bits, err

    @staticmethod
    def failure(bits: int, err: int) -> Optional[str]:
        """the message a batch with these status words fails with, or None"""
        if err:
            return f"ser_gru_v: a cluster wait gave up (error word {err}); the batch's recurrence is incomplete"
        if bits & 1:
            return "a value beyond the fp16 operand range (+-65504) reached the fusion head (use --mode fp32x)"
        return None


class FusionHead(_FusionBase):
    """The reference's bimodal fusion head (bin/train_cat_bimodal_lazy_1head.py:236-334, ``MultiModalEmotionClassifier``) on the device,
    over packed ragged batches: speech rows ``x1 [M1, D1]`` with ``offs1``, text rows ``x2 [M2, D2]`` with ``offs2`` -> ``[B, n_out]`` logits.
    EVERY UTTERANCE ALONE, as the reference's evaluation runs it (``batch_size=1``): no pad frame enters the recurrence, the attention or a
    pooling softmax, and a batch is arithmetically that batch-of-one loop (``head.evaluate``'s torch path pads to the batch's longest
    utterance instead).  ``forward`` enqueues on the current stream, outside the encoders' recorded tapes; per modality
      ser_pack_rows_flagged -> ser_gemm (projection) -> ser_layernorm_v (operand copy) -> ser_gemm (both directions' x W_ih^T) -> ser_gru_v
    then the four in-projection GEMMs (q of one side, packed k | v of the other, both ways), 2 x ser_xattn_mh_v (heads = 1), 2 x out-projection GEMM,
    2 x ser_attn_pool_v and ser_fusion_cls_v.  GEMM operand format: bf16 in mode "bf16", bf16 hi + lo in "fp32x", fp16 hi + lo otherwise;
    the recurrent product is always fp16 hi + lo."""
    NAMES = ("speech", "text")
    KEYS = FUSION_KEYS

    def __init__(self, state_dict, d1: int, d2: int, device="cuda:0", mode: str = "f16x", cluster: int = 0):
        self._init(state_dict, (d1, d2), (1, 1), device, mode, cluster)
        self.d1, self.d2 = d1, d2

    def forward(self, x1: torch.Tensor, offs1: Sequence[int], x2: torch.Tensor, offs2: Sequence[int], slot: int = 0,
                range_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[B, n_out]`` fp32 logits on the device (a view of the slot's buffer: valid until the slot's next ``forward``).  The fp16 range
        guard reports into ``range_flag`` (default: the slot's own word); ``status(slot)`` reads it and ser_gru_v's error word."""
        return self._forward((x1, x2), (offs1, offs2), slot, range_flag)


class TrimodalHead(_FusionBase):
    """The reference's trimodal fusion head (bin/train_cat_trimodal_lazy_1head.py, ``MultiModalEmotionClassifier`` over speech, text and a
    third feature stream, the ``prosody_*`` keys) on the device, every utterance alone (the ``batch_size=1`` of the reference's scoring
    scripts).  Three recurrences, three q and three k | v (N = 4 E) GEMMs, six ser_xattn_mh_v launches -- each attention module serves both
    of its query side's pairs, exactly as the reference shares them --, six out-projections (the second of a query side adds the first), three
    ser_attn_pool_v into a [B, 3 E] row and ser_fusion_cls_v with K = 3 E.  ``heads``: the head count of each module; a state dict does not
    record it, and the reference hard-codes (1, 1, 2)."""
    NAMES = ("speech", "text", "prosody")
    KEYS = TRIMODAL_KEYS

    def __init__(self, state_dict, d1: int, d2: int, d3: int, device="cuda:0", mode: str = "f16x", cluster: int = 0,
                 heads: Sequence[int] = (1, 1, 2)):
        self._init(state_dict, (d1, d2, d3), heads, device, mode, cluster)
        self.d1, self.d2, self.d3 = d1, d2, d3

    def forward(self, x1: torch.Tensor, offs1: Sequence[int], x2: torch.Tensor, offs2: Sequence[int], x3: torch.Tensor, offs3: Sequence[int],
                slot: int = 0, range_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[B, n_out]`` fp32 logits on the device (a view of the slot's buffer: valid until the slot's next ``forward``); ``x3`` may be
        ``[M3, D3, 1]`` (the reference squeezes the third stream's last axis)."""
        if isinstance(x3, torch.Tensor) and x3.dim() == 3 and x3.shape[-1] == 1:
            x3 = x3.squeeze(-1)
        return self._forward((x1, x2, x3), (offs1, offs2, offs3), slot, range_flag)


class DecodeResult:
    """One batch of ``WhisperDecoder.generate``: ``sequences`` int64 [B, n] (prompt, generated ids, eos / pad tail; n = the length at which
    every row had finished, else max_length), ``languages`` [B], ``lists`` (per utterance the generated ids without the prompt, up to and
    excluding eos), ``margins`` fp32 [B, n - 1] (top-1 minus top-2 masked logit of position p's decision, +inf where nothing was decided),
    ``range_bits`` (fp16 range guard) and ``err`` (ser_dec_select_v's error word): the batch failed when either is set.
    After ``generate(..., token_times=True)`` also ``token_times`` (per utterance fp32 seconds of its n generated tokens, the closing eos
    included: HF's ``token_timestamps`` behind the prompt; None where ``ts_status`` is set), ``token_frames`` (the n - 1 first frames) and
    ``ts_status`` (int32 [B]: ser_ts_matrix_v's status, SER_TS_NO_FRAMES, or ser_dtw_v's for an utterance of two rows or more): an
    utterance whose word is set fails ALONE.  ``ts_matrix``: the fp32 matrices on the device, [B, rows, pitch], until the next call.
    After a beam run (``generate(..., num_beams=K)``, K >= 2) ``sequences`` / ``lists`` / ``languages`` hold the best finished hypothesis
    of every utterance (its length comes from its own history), and also: ``nbest`` (per utterance up to K ``(generated ids, score)`` pairs,
    best first, the closing eos included), ``beam_scores`` float64 [B] (the best one's), ``beam_trace`` (dict: ``first`` = the position of the
    first beam step, ``run`` int32 [n, B, K, 2] and ``cand`` int32 [n, B, 2K, 2] = (parent, token) of the running rows and of the candidates
    of every position, ``cand_scores`` float64 [n, B, 2K], ``fin_scores`` / ``fin_handles`` / ``n_fin`` / ``flags`` / ``done_step``: the
    finished sets and flags as the device left them, ``run_scores`` float64 [B, K]) and ``beam_gaps`` float64 [n, B] (per position the
    smallest gap of a comparison that decided the step, +inf where none did).  ``margins`` then covers the prompt positions only.
    After a segment-timestamps run (``generate(..., timestamps=True)``) ``sequences`` / ``lists`` hold the timestamp tokens too (prompt
    ``[start, language, task]``), and also: ``segments`` (per utterance a list of ``(start_s, end_s, ids)``, ``transcribe.segments_of`` of
    its list), ``next_seek`` (int64 [B]: the frames HF's seek would advance by), ``ts_gaps`` float64 [B, n - 1] (ser_dec_select_ts_v's
    |L - M| of position p's decision, +inf where the sum rule compared nothing) and, with ``keep_logits``, ``step_logits`` (fp32
    [steps, B, V] on the device: the logits of every step from the first generated position on).
    After a scored run (``generate(..., scores=True)``, greedy or with ``timestamps``) also ``token_logprobs`` (per utterance float64
    [its generated tokens, the first eos included, nothing after it]: log-softmax of the processed row at the chosen token,
    ser_dec_select_score_v's), ``avg_logprob`` (float64 [B]: their sum in ascending order over their count, HF's
    ``_retrieve_avg_logprobs`` of a file given alone; NaN for an utterance without a generated token) and ``no_speech_prob`` (float64 [B]:
    softmax of the first decoder position's raw logits at ``spec.no_speech_token``; with ``keep_logits`` those logits stay in
    ``first_logits``, fp32 [B, V] on the device)."""

    token_times = token_frames = ts_status = ts_matrix = None
    token_logprobs = avg_logprob = no_speech_prob = first_logits = None
    nbest = beam_scores = beam_trace = beam_gaps = beam_logits = None
    segments = next_seek = ts_gaps = step_logits = None

    def __init__(self, sequences, languages, lists, margins, range_bits, err):
        self.sequences, self.languages, self.lists, self.margins = sequences, languages, lists, margins
        self.range_bits, self.err = int(range_bits), int(err)

    @property
    def failed(self) -> bool:
        return bool(self.range_bits & 1) or self.err != 0


class WhisperDecoder(_LaunchHost):
    """Whisper decoder with greedy short-form generation (HF modeling_whisper.py WhisperDecoder, generation_whisper.py with defaults) behind
    ``WhisperEncoder``: the reference's transcripts (test/Whisper transcriptions.ipynb).  Lock-step: all rows of a batch stand at the same
    position; one step takes ids[:, pos] to ids[:, pos + 1] on the device -- ids, finished flags and the position live there, and the
    host reads the count of unfinished rows back every ``CHECK_EVERY`` steps only.  A step is 11 launches per layer (3 LayerNorms, 6 GEMMs,
    2 ser_dec_attn_v) + 4, recorded once per (slot, B) and replayed with ser_run; the host leaves the logits launches out at positions
    whose next token is forced.  The cross keys / values of all layers are projected once per batch into an fp32 cache."""

    DEC_MODES = ("f16x", "fp32x", "bf16")
    CHECK_EVERY = 4
    PHASE_STEADY, PHASE_FIRST, PHASE_LANG = 0, 1, 2

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "f16x", spec=None):
        if mode not in self.DEC_MODES:
            print(f"WhisperDecoder: mode '{mode}' has no decoder form, using 'f16x'")
            mode = "f16x"
        m = MODES[mode]
        super().__init__(device, mode, m, m, mode == "f16x" and _os.environ.get("SER_NO_RANGE_GUARD", "0") != "1")
        if geo.family != FAMILY_WHISPER or geo.decoder_layers < 1:
            raise ValueError("WhisperDecoder needs a whisper geometry with decoder_layers >= 1")
        if geo.hidden != 64 * geo.decoder_attention_heads:
            raise ValueError("the decoder attention kernel needs head dim 64 (every Whisper size)")
        self.geo, self.spec = geo, spec
        sd = state_dict
        D, V = geo.hidden, geo.decoder_vocab_size
        self.Vp = (V + 7) // 8 * 8                      # GEMM N: zero rows behind the vocabulary; their logits are never read
        emb = torch.zeros((self.Vp, D), dtype=torch.float32)
        emb[:V] = sd["decoder.embed_tokens.weight"].detach().float().cpu()
        self.embed = self._dev_f32(emb)
        self.proj = self._linear(emb, None, name="decoder.embed_tokens.weight")        # tied output projection, no bias
        self.pos_emb = self._dev_f32(sd["decoder.embed_positions.weight"])
        if self.pos_emb.shape[0] != geo.max_target_positions:
            raise ValueError("decoder.embed_positions.weight does not have max_target_positions rows")
        self.final_ln = self._ln(sd, "decoder.layer_norm")
        self.layers = []
        zeros = torch.zeros(D)
        for i in range(geo.decoder_layers):
            p = f"decoder.layers.{i}"
            sa, ca = p + ".self_attn", p + ".encoder_attn"
            cat = lambda names: torch.cat([sd[n].detach().float().cpu() for n in names], 0)
            lay = dict(
                ln1=self._ln(sd, p + ".self_attn_layer_norm"),
                qkv=self._linear(cat([sa + ".q_proj.weight", sa + ".k_proj.weight", sa + ".v_proj.weight"]),       # k_proj has no bias
                                 torch.cat([sd[sa + ".q_proj.bias"].float().cpu(), zeros, sd[sa + ".v_proj.bias"].float().cpu()]),
                                 name=sa + ".{q,k,v}_proj.weight"),
                out=self._linear(sd[sa + ".out_proj.weight"], sd[sa + ".out_proj.bias"], name=sa + ".out_proj.weight"),
                ln2=self._ln(sd, p + ".encoder_attn_layer_norm"),
                cq=self._linear(sd[ca + ".q_proj.weight"], sd[ca + ".q_proj.bias"], name=ca + ".q_proj.weight"),
                ckv=self._linear(cat([ca + ".k_proj.weight", ca + ".v_proj.weight"]), torch.cat([zeros, sd[ca + ".v_proj.bias"].float().cpu()]),
                                 name=ca + ".{k,v}_proj.weight"),
                cout=self._linear(sd[ca + ".out_proj.weight"], sd[ca + ".out_proj.bias"], name=ca + ".out_proj.weight"),
                ln3=self._ln(sd, p + ".final_layer_norm"),
                fc1=self._linear(sd[p + ".fc1.weight"], sd[p + ".fc1.bias"], name=p + ".fc1.weight"),
                fc2=self._linear(sd[p + ".fc2.weight"], sd[p + ".fc2.bias"], name=p + ".fc2.weight"))
            self.layers.append(lay)
        self._plans: Dict = {}
        self._masks: Dict = {}
        self._cache, self._cache_B, self._cache_rows = None, 0, 0

    def _ln(self, sd, prefix):
        return (self._dev_f32(sd[prefix + ".weight"]), self._dev_f32(sd[prefix + ".bias"]))

    # ------------------------------------------------------------------ buffers
    def _plan(self, B: int, slot: int, heads=None, beams: int = 1, timestamps: bool = False, scores: bool = False):
        """``heads``: the alignment heads of the capture variant of the step (``generate(token_times=True)``), part of the plan's key; the
        default plan (None) records exactly the launches it always did.  ``beams`` K >= 2: the beam plan, keyed (slot, B, "beam", K).
        ``timestamps``: the segment-timestamps plan, keyed (slot, B, "ts"), whose step ends in ser_dec_select_ts_v.  ``scores``: the
        scored forms of the greedy and the timestamps plan, keyed (slot, B, "score") and (slot, B, "ts", "score"), whose step ends in
        ser_dec_select_score_v; the unscored plans record what they always did."""
        if beams > 1:
            return self._beam_plan(B, slot, beams)
        key = (slot, B) if heads is None else (slot, B, tuple(heads))
        if timestamps:
            key = (slot, B, "ts")
        if scores:
            key = (slot, B, "ts", "score") if timestamps else (slot, B, "score")
        pl = self._plans.get(key)
        if pl is not None:
            return pl
        geo, dev = self.geo, self.device
        D, L, T, S = geo.hidden, geo.decoder_layers, geo.max_target_positions, geo.max_source_positions
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        pl = dict(B=B, ids=i32(B, T), finished=i32(B), margin=f32(B, T), pos=i32(1), unfinished=i32(1), work=i32(2), err=i32(1),
                  phase=i32(T), forced=i32(T), range_flag=i32(1) if self.fp16_planes else None,
                  x=[f32(B, D), f32(B, D), f32(B, D)], qkv=f32(B, 3 * D), qc=f32(B, D), logits=f32(B, self.Vp),
                  xa=self._new_act(B, D), ctx=self._new_act(B, D), ffn=self._new_act(B, geo.decoder_ffn_dim),
                  enc_act=self._new_act(B * S, D))
        # the K / V caches (at large-v3 geometry and B = 16: 2.3 GB self + 7.9 GB cross) belong to the decoder, not to the plan: generate()
        # ends with a host synchronisation, so no two batches are ever in flight and every (slot, B) plan can read the same storage
        ks, vs, cr = self._caches(B)
        pl["kself"], pl["vself"] = ks[: L * B * T * D].view(L, B, T, D), vs[: L * B * T * D].view(L, B, T, D)
        pl["cross"] = cr[: L * B * S * 2 * D].view(L, B * S, 2 * D)
        pl["host"] = torch.empty(3, dtype=torch.int32).pin_memory()
        pl["heads"] = None
        if timestamps:
            pl["timestamps"] = True
            pl["ts_gap"] = torch.empty((B, T), dtype=torch.float64, device=dev)
        if scores:
            pl["scores"] = True
            pl["score_blob"] = torch.empty(B * T + B, dtype=torch.float64, device=dev)      # logprob [B, T] | no_speech [B]: one copy back
        if heads is not None:
            heads = tuple((int(l), int(h)) for l, h in heads)
            if not 1 <= len(heads) <= _lib.TS_MAX_HEADS or any(not (0 <= l < L and 0 <= h < geo.decoder_attention_heads) for l, h in heads):
                raise ValueError(f"alignment_heads {heads} do not fit {L} decoder layers of {geo.decoder_attention_heads} heads "
                                 f"(at most {_lib.TS_MAX_HEADS} pairs)")
            if T - 1 > _lib.TS_THREADS or S > _lib.TS_MAX_KEYS:
                raise ValueError(f"token times take up to {_lib.TS_THREADS} token rows and {_lib.TS_MAX_KEYS} keys")
            pl["heads"] = heads
            pl["keep"] = f32(T, B, len(heads), 64)              # the alignment heads' cross queries of every position
            pl["ts_tab"] = TableBlob(B, 2, dev)                 # token rows | frames (int32)
            pl["ts_out"] = i32(2 * B + B * T)                   # matrix status | DTW status | first frames [B, T]: one copy back
            pl["ts_host"] = torch.empty(2 * B + B * T, dtype=torch.int32).pin_memory()
        self._flag = None if pl["range_flag"] is None else pl["range_flag"].data_ptr()
        pl["tape"] = tape = Tape()
        with self._launching(tape):
            self._step_launches(pl)
        if len(self._plans) >= 6:
            self._plans.pop(next(iter(self._plans)))
        self._plans[key] = pl
        return pl

    def _beam_plan(self, Bu: int, slot: int, K: int):
        """The plan of a beam run: B K rows (row b K + k is beam k of utterance b) over a self cache of B K physical rows read through the
        ancestor table, the B utterances' cross cache shared by their K rows, and the beam state in ONE device blob that comes back
        with one copy.  pl["B"] is the row count, as every launch of the step reads it; pl["Bu"] the utterances."""
        key = (slot, Bu, "beam", K)
        pl = self._plans.get(key)
        if pl is not None:
            return pl
        geo, dev = self.geo, self.device
        D, L, T, S, V = geo.hidden, geo.decoder_layers, geo.max_target_positions, geo.max_source_positions, geo.decoder_vocab_size
        B = Bu * K
        work_bytes = int(lib.ser_beam_work_bytes(Bu, K, V))
        if work_bytes < 0:
            raise ValueError(f"beam search takes 2..{_lib.BEAM_MAX_K} beams over a vocabulary of at least 2 K tokens (K={K}, V={V})")
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        pl = dict(B=B, Bu=Bu, K=K, ids=i32(B, T), finished=i32(B), margin=f32(B, T), pos=i32(1), unfinished=i32(1), work=i32(2), err=i32(1),
                  phase=i32(T), forced=i32(T), range_flag=i32(1) if self.fp16_planes else None,
                  x=[f32(B, D), f32(B, D), f32(B, D)], qkv=f32(B, 3 * D), qc=f32(B, D), logits=f32(B, self.Vp),
                  xa=self._new_act(B, D), ctx=self._new_act(B, D), ffn=self._new_act(B, geo.decoder_ffn_dim),
                  enc_act=self._new_act(Bu * S, D))
        ks, vs, cr = self._caches(Bu, B)
        pl["kself"], pl["vself"] = ks[: L * B * T * D].view(L, B, T, D), vs[: L * B * T * D].view(L, B, T, D)
        pl["cross"] = cr[: L * Bu * S * 2 * D].view(L, Bu * S, 2 * D)
        pl["heads"] = None
        # the beam state: float64 parts first, then int32 ones, each 8-byte aligned: ONE blob, so that one copy brings all of it back
        parts = (("run", np.float64, (Bu, K)), ("fin_score", np.float64, (Bu, K)), ("cand_score", np.float64, (T, Bu, 2 * K)),
                 ("gaps", np.float64, (T, Bu)), ("fin_handle", np.int32, (Bu, K, 2)), ("state", np.int32, (Bu, 4)),
                 ("trace_run", np.int32, (T, Bu, K, 2)), ("trace_cand", np.int32, (T, Bu, 2 * K, 2)))
        off, lay = 0, {}
        for name, dt, shape in parts:
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            lay[name] = (off, dt, shape)
            off += (n + 7) // 8 * 8
        pl["beam_layout"], pl["beam_bytes"] = lay, off
        pl["beam_blob"] = torch.zeros(off, dtype=torch.uint8, device=dev)
        pl["beam_host"] = torch.empty(off, dtype=torch.uint8).pin_memory()
        pl["beam_init"] = torch.empty(off, dtype=torch.uint8).pin_memory()         # what begin() uploads: zeros, run = [0, -inf ..], flag = 1
        pl["src"] = i32(2, B, T)                        # the ancestor table, both halves
        pl["src_init"] = torch.arange(B, dtype=torch.int32, device=dev).view(1, B, 1).expand(2, B, T).contiguous()
        pl["lenpow"] = torch.zeros(T + 1, dtype=torch.float64, device=dev)
        pl["beam_ticket"] = i32(2)
        pl["beam_work"] = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device=dev)
        pl["beam_work_bytes"] = work_bytes
        pl["host"] = torch.empty(3, dtype=torch.int32).pin_memory()
        self._flag = None if pl["range_flag"] is None else pl["range_flag"].data_ptr()
        pl["tape"] = tape = Tape()
        with self._launching(tape):
            self._step_launches(pl)
        if len(self._plans) >= 6:
            self._plans.pop(next(iter(self._plans)))
        self._plans[key] = pl
        return pl

    def _keep_q(self, pl, layer: int, qc: torch.Tensor) -> None:
        """The capture of the step (ser_dec_keep_q_v): one launch per run of alignment heads that lie in ``layer``, after its cross q
        projection."""
        heads = pl["heads"]
        geo = self.geo
        k = 0
        while k < len(heads):
            if heads[k][0] != layer:
                k += 1
                continue
            e = k
            while e < len(heads) and heads[e][0] == layer and e - k < _lib.TS_KEEP_HEADS:
                e += 1
            a = self._cmd("dec_keep_q")
            a.q, a.ldq, a.pos, a.keep = qc.data_ptr(), geo.hidden, pl["pos"].data_ptr(), pl["keep"].data_ptr()
            for j in range(k, e):
                a.head[j - k] = heads[j][1]
            a.n_heads, a.slot0, a.n_align, a.B, a.H, a.max_pos = e - k, k, len(heads), pl["B"], geo.decoder_attention_heads, geo.max_target_positions
            self._issue(_lib.OP_DEC_KEEP_Q, a, "ser_dec_keep_q")
            k = e

    def _caches(self, B: int, rows: Optional[int] = None):
        """(self k, self v, cross k | v) flat fp32 storage for the largest batch seen.  A larger batch replaces it and drops every plan,
        whose recorded commands point into the old storage.  ``rows``: the rows of the self cache when they are not the B utterances (a
        beam plan's B K); the cross cache is per utterance."""
        geo = self.geo
        rows = B if rows is None else rows
        if B > self._cache_B or rows > self._cache_rows:
            self._plans.clear()
            self._cache = None                          # free before allocating the larger one
            B, rows = max(B, self._cache_B), max(rows, self._cache_rows)
            n_self = geo.decoder_layers * rows * geo.max_target_positions * geo.hidden
            n_cross = geo.decoder_layers * B * geo.max_source_positions * 2 * geo.hidden
            self._cache = tuple(torch.empty(n, dtype=torch.float32, device=self.device) for n in (n_self, n_self, n_cross))
            self._cache_B, self._cache_rows = B, rows
        return self._cache

    def _dec_attn(self, pl, q: torch.Tensor, ldq: int, kc: torch.Tensor, vc_ptr: int, ldc: int, batch_stride: int, max_len: int, *,
                  new=None, lens=None, len_add: int) -> None:
        geo = self.geo
        if pl.get("K"):                                 # a beam plan: the same arguments behind the ancestor table or the row divisor
            x = self._cmd("dec_attn_beam")
            a = x.base
            if new is not None:
                x.src, x.src_parity_stride, x.ld_src = pl["src"].data_ptr(), pl["src"].stride(0), pl["src"].shape[2]
            x.row_div = 1 if new is not None else pl["K"]
        else:
            x = None
            a = self._cmd("dec_attn")
        a.q, a.ldq = q.data_ptr(), ldq
        if new is not None:
            a.k_new, a.v_new, a.ld_new = new
        a.kcache, a.vcache, a.ldc, a.batch_stride = kc.data_ptr(), vc_ptr, ldc, batch_stride
        a.lens, a.lens_stride, a.len_add = _ptr(lens), 0, len_add
        ctx = pl["ctx"]
        a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = ctx.ptr, ctx.cols, ctx.plane_stride, self._flag
        a.scale, a.B, a.H, a.dh, a.max_len, a.mode = 64 ** -0.5, pl["B"], geo.decoder_attention_heads, 64, max_len, self.mode
        if x is not None:
            self._issue(_lib.OP_DEC_ATTN_BEAM, x, "ser_dec_attn_beam")
            return
        self._issue(_lib.OP_DEC_ATTN, a, "ser_dec_attn")

    def _step_launches(self, pl) -> None:
        """One decode step: ids[:, pos] -> logits -> ids[:, pos + 1].  pl["n_body"] / pl["n_logits"]: the command ranges of the layers and
        of final LayerNorm + logits GEMM (left out when the next token is forced); ser_dec_select_v is the last command."""
        geo = self.geo
        B, D, T, S = pl["B"], geo.hidden, geo.max_target_positions, geo.max_source_positions
        x0, x1, x2 = pl["x"]
        e = self._cmd("dec_embed")
        e.ids, e.ld_ids, e.pos = pl["ids"].data_ptr(), T, pl["pos"].data_ptr()
        e.embed_tokens, e.embed_positions, e.out, e.ldo = self.embed.data_ptr(), self.pos_emb.data_ptr(), x0.data_ptr(), D
        e.B, e.D, e.vocab, e.max_pos = B, D, geo.decoder_vocab_size, T
        self._issue(_lib.OP_DEC_EMBED, e, "ser_dec_embed")
        qkv, qc = pl["qkv"], pl["qc"]
        for i, lay in enumerate(self.layers):
            self._layernorm(x0, D, lay["ln1"], B, D, out_act=pl["xa"])
            self._gemm(pl["xa"], lay["qkv"], B, out_f32=qkv, ldo_f32=3 * D)
            self._dec_attn(pl, qkv, 3 * D, pl["kself"][i], pl["vself"][i].data_ptr(), D, T * D, T,
                           new=(qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D), lens=pl["pos"], len_add=1)
            self._gemm(pl["ctx"], lay["out"], B, residual=x0, ldr=D, out_f32=x1, ldo_f32=D)
            self._layernorm(x1, D, lay["ln2"], B, D, out_act=pl["xa"])
            self._gemm(pl["xa"], lay["cq"], B, out_f32=qc, ldo_f32=D)
            if pl["heads"] is not None:
                self._keep_q(pl, i, qc)
            cross = pl["cross"][i]
            self._dec_attn(pl, qc, D, cross, cross.data_ptr() + 4 * D, 2 * D, S * 2 * D, S, len_add=S)
            self._gemm(pl["ctx"], lay["cout"], B, residual=x1, ldr=D, out_f32=x2, ldo_f32=D)
            self._layernorm(x2, D, lay["ln3"], B, D, out_act=pl["xa"])
            self._gemm(pl["xa"], lay["fc1"], B, act=_lib.ACT_GELU, out_act=pl["ffn"])
            self._gemm(pl["ffn"], lay["fc2"], B, residual=x2, ldr=D, out_f32=x0, ldo_f32=D)
        pl["n_body"] = self._rec.n if self._rec is not None else None
        self._layernorm(x0, D, self.final_ln, B, D, out_act=pl["xa"])
        self._gemm(pl["xa"], self.proj, B, out_f32=pl["logits"], ldo_f32=self.Vp)
        pl["n_logits"] = self._rec.n if self._rec is not None else None
        q = self._cmd("dec_select_score") if pl.get("scores") else None
        x = q.ts if q is not None else (self._cmd("dec_select_ts") if pl.get("timestamps") else None)
        s = self._cmd("dec_select") if x is None else x.base
        s.logits, s.ldl = pl["logits"].data_ptr(), self.Vp
        s.mask, s.ldm = 0, geo.decoder_vocab_size                      # the spec's masks: set per generate() call (_bind_spec)
        s.phase, s.forced = pl["phase"].data_ptr(), pl["forced"].data_ptr()
        s.ids, s.ld_ids, s.finished = pl["ids"].data_ptr(), T, pl["finished"].data_ptr()
        s.margin, s.ld_margin = pl["margin"].data_ptr(), T
        s.pos, s.unfinished, s.work, s.err = pl["pos"].data_ptr(), pl["unfinished"].data_ptr(), pl["work"].data_ptr(), pl["err"].data_ptr()
        s.B, s.V, s.eos, s.pad, s.max_pos = B, geo.decoder_vocab_size, 0, 0, T
        pl["select"] = s
        if q is not None:
            blob = pl["score_blob"]
            q.logprob, q.ld_logprob, q.no_speech = blob.data_ptr(), T, blob.data_ptr() + 8 * B * T
            q.no_speech_token, q.rule = 0, 1 if pl.get("timestamps") else 0
            if q.rule:
                x.ts_gap, x.ld_gap = pl["ts_gap"].data_ptr(), T
                x.ts_begin, x.no_ts, x.begin_index, x.max_initial = 1, 0, 1, -1
                pl["select_ts"] = x
            pl["select_score"] = q
            self._issue(_lib.OP_DEC_SELECT_SCORE, q, "ser_dec_select_score")
            return
        if x is not None:
            # the spec's token layout (begin): placeholders that pass the launcher's checks while the step is recorded
            x.ts_gap, x.ld_gap = pl["ts_gap"].data_ptr(), T
            x.ts_begin, x.no_ts, x.begin_index, x.max_initial = 1, 0, 1, -1
            pl["select_ts"] = x
            self._issue(_lib.OP_DEC_SELECT_TS, x, "ser_dec_select_ts")
            return
        self._issue(_lib.OP_DEC_SELECT, s, "ser_dec_select")
        if pl.get("K"):
            # the second tail of a beam plan: from the first generated position the step ends with ser_beam_select_v instead
            # (_run_step replays the tail the position needs)
            pl["n_select"] = self._rec.n if self._rec is not None else None
            K, Bu, lay = pl["K"], pl["Bu"], pl["beam_layout"]
            at = lambda name: pl["beam_blob"].data_ptr() + lay[name][0]
            g = self._cmd("beam_select")
            g.logits, g.ldl, g.mask, g.ldm = pl["logits"].data_ptr(), self.Vp, 0, geo.decoder_vocab_size
            g.phase, g.lenpow, g.ids, g.ld_ids = pl["phase"].data_ptr(), pl["lenpow"].data_ptr(), pl["ids"].data_ptr(), T
            g.src, g.src_parity_stride, g.ld_src = pl["src"].data_ptr(), pl["src"].stride(0), T
            g.run, g.fin_score, g.fin_handle, g.state = at("run"), at("fin_score"), at("fin_handle"), at("state")
            g.trace_run, g.trace_cand, g.cand_score, g.gaps = at("trace_run"), at("trace_cand"), at("cand_score"), at("gaps")
            g.work, g.work_bytes = pl["beam_work"].data_ptr(), pl["beam_work_bytes"]
            g.pos, g.unfinished, g.ticket, g.err = pl["pos"].data_ptr(), pl["unfinished"].data_ptr(), pl["beam_ticket"].data_ptr(), pl["err"].data_ptr()
            g.B, g.K, g.V, g.eos, g.pad, g.max_pos = Bu, K, geo.decoder_vocab_size, 0, 0, T
            g.max_length, g.prompt_len = T, 1                                 # the spec's: set per generate() call (begin)
            pl["beam_select"] = g
            self._issue(_lib.OP_BEAM_SELECT, g, "ser_beam_select")

    def _spec_masks(self, spec) -> torch.Tensor:
        """fp32 [3, V] additive masks of a spec on the device: steady, first generated position, language set."""
        key = (spec.suppress_tokens, spec.begin_suppress_tokens, spec.lang_ids)
        m = self._masks.get(key)
        if m is None:
            V = self.geo.decoder_vocab_size
            bad = [t for t in key[0] + key[1] + key[2] if not 0 <= t < V]
            if bad:
                raise ValueError(f"generation spec names token ids outside the vocabulary: {bad[:4]}")
            h = torch.zeros((3, V), dtype=torch.float32)
            h[0, list(spec.suppress_tokens)] = float("-inf")
            h[1] = h[0]
            h[1, list(spec.begin_suppress_tokens)] = float("-inf")
            h[2] = float("-inf")
            h[2, list(spec.lang_ids)] = 0.0
            m = self._masks[key] = h.to(self.device)
        return m

    # ------------------------------------------------------------------ the batch
    @_on_stream
    def project_cross(self, pl, enc_last: torch.Tensor) -> None:
        """Once per batch: the encoder's last hidden state [B * 1500, D] -> every layer's cross keys | values (one ser_gemm per layer, N = 2 D)
        in the fp32 cache."""
        geo = self.geo
        B, D, S = pl.get("Bu", pl["B"]), geo.hidden, geo.max_source_positions      # a beam plan's rows share their utterance's cross cache
        if tuple(enc_last.shape) != (B * S, D) or enc_last.dtype != torch.float32 or not enc_last.is_contiguous():
            raise ValueError(f"the decoder needs the encoder's last hidden state as contiguous fp32 [{B * S}, {D}], got {tuple(enc_last.shape)}")
        ea = pl["enc_act"]
        check(lib.ser_pack_rows_flagged(enc_last.data_ptr(), D, 1, B * S, D, 0, ea.ptr, D, ea.plane_stride, self.mode, self._flag, self._s()),
              "ser_pack_rows_flagged")
        for i, lay in enumerate(self.layers):
            self._gemm(ea, lay["ckv"], B * S, out_f32=pl["cross"][i], ldo_f32=2 * D)

    def _run_step(self, pl, with_logits: bool, beam: bool = False) -> None:
        tape = pl["tape"]
        st = self._s()
        if pl.get("K"):
            # a beam plan ends with two tails, [.. logits | ser_dec_select_v | ser_beam_select_v]: the prompt steps take the first (all B K
            # rows are identical and choose alike), the generated positions the second
            cmd_at = lambda i: C.byref(tape.cmds, i * C.sizeof(_lib.Cmd))
            rc = lib.ser_run(tape.cmds, pl["n_logits"] if with_logits or beam else pl["n_body"], C.byref(tape._failed), st)
            if rc == 0:
                first = pl["n_select"] if beam else pl["n_logits"]
                rc = lib.ser_run(cmd_at(first), 1, C.byref(tape._failed), st)
                if rc != 0:
                    tape._failed.value += first
            if rc != 0:
                check(rc, f"ser_run (decoder beam step, command {tape._failed.value})")
            return
        if with_logits:
            rc = lib.ser_run(tape.cmds, tape.n, C.byref(tape._failed), st)
        else:
            rc = lib.ser_run(tape.cmds, pl["n_body"], C.byref(tape._failed), st)
            if rc == 0:
                rc = lib.ser_run(C.byref(tape.cmds, pl["n_logits"] * C.sizeof(_lib.Cmd)), tape.n - pl["n_logits"], C.byref(tape._failed), st)
        if rc != 0:
            check(rc, f"ser_run (decoder step, command {tape._failed.value})")

    def begin(self, B: int, spec=None, language=None, slot: int = 0, forced_ids=None, token_times: bool = False, num_beams: int = 1,
              length_penalty: float = 1.0, timestamps: bool = False, scores: bool = False):
        """Reset the slot's decoding state for a batch of B: ids[:, 0] = start, position 0, nothing finished.  ``forced_ids`` (tests:
        teacher forcing): a whole id row to follow instead of the spec's prompt.  ``token_times``: the capture variant of the step.
        ``num_beams`` K >= 2: the beam plan (B K rows) with its state reset: running scores [0, -inf, ..], empty finished sets, flags up,
        the identity ancestor table.  ``timestamps``: the segment-timestamps plan and its prompt ``[start, language, task]``; with
        ``forced_ids`` the rule still counts its generated tokens from position 3.  ``scores``: the scored form of the greedy or the
        timestamps plan (ser_dec_select_score_v), its log-probabilities reset to +inf and its no-speech probabilities to NaN."""
        spec = spec or self.spec
        if spec is None:
            raise ValueError("WhisperDecoder needs a GenerationSpec")
        if scores and (token_times or num_beams > 1):
            raise ValueError("scores=True does not go with " + ("token_times" if token_times else "num_beams > 1") + ": not built")
        if timestamps and (token_times or num_beams > 1):
            raise ValueError("timestamps=True does not go with " + ("token_times" if token_times else "num_beams > 1") + ": not built")
        geo = self.geo
        T = geo.max_target_positions
        n_max = min(int(spec.max_length), T)
        P = spec.prompt_len(timestamps)
        if scores:
            pl = self._plan(B, slot, timestamps=timestamps, scores=True)
        else:
            pl = self._plan(B, slot, spec.require_alignment_heads() if token_times else None, beams=num_beams, timestamps=timestamps)
        language = spec.language if language is None else language
        forced = np.full(T, -1, dtype=np.int32)
        phase = np.zeros(T, dtype=np.int32)
        if forced_ids is not None:
            forced[: len(forced_ids) - 1] = np.asarray(forced_ids[1:], dtype=np.int32)
            start = int(forced_ids[0])
        else:
            start = spec.decoder_start_token_id
            forced[1] = spec.task_id
            if not timestamps:
                forced[2] = spec.no_timestamps_token_id
            if language is not None:
                forced[0] = int(language)
            phase[0], phase[P - 1] = self.PHASE_LANG, self.PHASE_FIRST
        pl["forced_host"], pl["n_max"], pl["spec"], pl["P"] = forced, n_max, spec, P
        pl["forced"].copy_(torch.from_numpy(forced))
        pl["phase"].copy_(torch.from_numpy(phase))
        for k in ("finished", "pos", "unfinished", "work", "err") + (("range_flag",) if pl["range_flag"] is not None else ()):
            pl[k].zero_()
        pl["ids"].zero_()
        pl["ids"][:, 0] = start
        pl["margin"].fill_(float("inf"))
        s = pl["select"]
        s.mask, s.eos, s.pad = self._spec_masks(spec).data_ptr(), spec.eos_token_id, spec.pad_token_id
        self._flag = None if pl["range_flag"] is None else pl["range_flag"].data_ptr()
        if timestamps:
            V = geo.decoder_vocab_size
            initial = spec.max_initial_timestamp_index
            if not 0 < spec.timestamp_begin < V or not 0 <= spec.eos_token_id < V:
                raise ValueError(f"segment timestamps need timestamp tokens behind no_timestamps_token_id={spec.no_timestamps_token_id} "
                                 f"and eos inside the vocabulary of {V}")
            x = pl["select_ts"]
            x.ts_begin, x.no_ts, x.begin_index = spec.timestamp_begin, spec.no_timestamps_token_id, P
            x.max_initial = -1 if initial is None else int(initial)
            pl["ts_gap"].fill_(float("inf"))
        if scores:
            if not 0 <= spec.no_speech_token < geo.decoder_vocab_size:
                raise ValueError(f"scores need the no-speech token {spec.no_speech_token} inside the vocabulary of {geo.decoder_vocab_size}")
            pl["select_score"].no_speech_token = spec.no_speech_token
            pl["score_blob"][: B * T].fill_(float("inf"))
            pl["score_blob"][B * T:].fill_(float("nan"))
        if pl.get("K"):
            from .beam import lenpow_table
            if n_max <= spec.PROMPT_LEN:
                raise ValueError(f"beam search needs max_length > {spec.PROMPT_LEN} (the prompt)")
            K, lay = pl["K"], pl["beam_layout"]
            g = pl["beam_select"]
            g.mask, g.eos, g.pad, g.max_length, g.prompt_len = s.mask, spec.eos_token_id, spec.pad_token_id, n_max, spec.PROMPT_LEN
            init = pl["beam_init"].numpy()
            init[:] = 0
            view = lambda name: init[lay[name][0]: lay[name][0] + int(np.prod(lay[name][2])) * np.dtype(lay[name][1]).itemsize].view(lay[name][1]).reshape(lay[name][2])
            run = view("run")
            run[:], run[:, 0] = -np.inf, 0.0
            view("state")[:, 1] = 1
            view("gaps")[:] = np.inf
            pl["beam_blob"].copy_(pl["beam_init"], non_blocking=True)
            pl["lenpow"].copy_(torch.from_numpy(lenpow_table(T + 1, length_penalty)))
            pl["src"].copy_(pl["src_init"])
            pl["beam_ticket"].zero_()
            pl["length_penalty"] = float(length_penalty)
        return pl

    @_on_stream
    def generate(self, enc_last: torch.Tensor, B: int, spec=None, language=None, slot: int = 0, token_times: bool = False,
                 lengths: Optional[Sequence[int]] = None, num_beams: Optional[int] = None, length_penalty: Optional[float] = None,
                 keep_logits: bool = False, timestamps: bool = False, num_frames: Optional[Sequence[int]] = None,
                 scores: bool = False) -> DecodeResult:
        """Greedy transcription of a batch from the encoder's last hidden state (fp32 [B * 1500, D], e.g. ``HiddenStates.states[-1]``).
        ``token_times``: also HF's ``token_timestamps`` of every utterance given alone (``DecodeResult.token_times``), from the alignment
        heads' cross-attention; needs ``lengths``, the utterances' sample counts (HF's ``num_frames`` = length // 160).
        ``num_beams`` / ``length_penalty``: None takes the spec's; 1 is the greedy path and its plan, untouched; K >= 2 is HF's beam search
        (early_stopping = False) on the device.  ``keep_logits`` (tests): a beam run keeps the fp32 logits of every beam step in
        ``DecodeResult.beam_logits`` [n, B K, V] on the device.
        ``timestamps``: the model's own segment times (HF's ``return_timestamps=True`` for one 30 s window): the prompt is
        ``[start, language, task]``, the step ends in ser_dec_select_ts_v on a plan of its own, and the result has ``segments``,
        ``next_seek`` and ``ts_gaps``; ``lengths`` (sample counts) bound the window, absent: the whole 30 s.  ``keep_logits`` then
        keeps ``DecodeResult.step_logits``.  ``num_frames`` (with ``timestamps``; the long-form loop): the mel frames of each row's window,
        given to ``segments_of`` as they are instead of ``lengths``' len // 160.  Does not go with ``token_times`` or ``num_beams > 1``.
        ``scores``: the greedy or the timestamps run on a scored plan of its own (the step ends in ser_dec_select_score_v, and the step
        at position 0 computes its logits even when the language is forced: the no-speech probability reads them); tokens, margins and
        ts_gaps are those of the unscored run, and the result also has ``token_logprobs``, ``avg_logprob`` and ``no_speech_prob``, read
        back once after the loop.  Does not go with ``token_times`` or ``num_beams > 1`` (a beam run returns ``beam_scores``)."""
        sp = spec or self.spec
        K = int(getattr(sp, "num_beams", 1) if num_beams is None else num_beams)
        if not 1 <= K <= _lib.BEAM_MAX_K:
            raise ValueError(f"num_beams={K} (1..{_lib.BEAM_MAX_K})")
        if scores and token_times:
            raise ValueError("scores=True with token_times: transcript scores with token times are not built")
        if scores and K > 1:
            raise ValueError("scores=True with num_beams > 1: transcript scores with beam search are not built (beam_scores are returned)")
        if timestamps and token_times:
            raise ValueError("timestamps=True with token_times: segment timestamps with token times are not built")
        if timestamps and K > 1:
            raise ValueError("timestamps=True with num_beams > 1: segment timestamps with beam search are not built")
        if timestamps and lengths is not None and len(lengths) != B:
            raise ValueError("lengths: one sample count per utterance")
        if num_frames is not None and (not timestamps or len(num_frames) != B or lengths is not None):
            raise ValueError("num_frames: one frame count per row of a timestamps run, in place of lengths")
        if K > 1:
            if token_times:
                raise ValueError("token times with beam search are not built: run with num_beams=1")
            lp = float(getattr(sp, "length_penalty", 1.0) if length_penalty is None else length_penalty)
            return self._generate_beams(enc_last, B, spec, language, slot, K, lp, keep_logits)
        if token_times and (lengths is None or len(lengths) != B):
            raise ValueError("token times need the sample count of every utterance (lengths)")
        if scores:
            pl = self.begin(B, spec, language, slot, timestamps=timestamps, scores=True)
        else:
            pl = self.begin(B, spec, language, slot, token_times=token_times, timestamps=timestamps)
        spec = pl["spec"]
        self.project_cross(pl, enc_last)
        n_max, forced, P = pl["n_max"], pl["forced_host"], pl["P"]
        host = pl["host"]
        kept = [] if keep_logits and (timestamps or scores) else None
        first_logits = None
        V = self.geo.decoder_vocab_size
        steps = 0
        for pos in range(n_max - 1):
            self._run_step(pl, with_logits=forced[pos] < 0 or (scores and pos == 0))
            steps += 1
            if kept is not None and pos >= P - 1:
                kept.append(pl["logits"][:, :V].clone())
            if kept is not None and scores and pos == 0:
                first_logits = pl["logits"][:, :V].clone()
            if steps % self.CHECK_EVERY == 0 and pos >= P - 1:
                host[0:1].copy_(pl["unfinished"], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                if int(host[0]) == 0:
                    break
        res = self.result(pl, steps)
        if kept is not None and scores:
            res.first_logits = first_logits
        if token_times:
            self._token_times(pl, res, lengths)
        if timestamps:
            from .transcribe import segments_of, window_frames
            res.ts_gaps = pl["ts_gap"][:, : res.sequences.shape[1] - 1].cpu().numpy()
            res.segments, res.next_seek = [], np.zeros(B, dtype=np.int64)
            for b, ids in enumerate(res.lists):
                nf = int(num_frames[b]) if num_frames is not None else window_frames(None if lengths is None else lengths[b])
                segs, adv = segments_of(ids, spec.timestamp_begin, nf)
                res.segments.append(segs)
                res.next_seek[b] = adv
        if kept is not None:
            res.step_logits = torch.stack(kept) if kept else None
        if scores:
            self._scores(pl, res)
        return res

    def _scores(self, pl, res: DecodeResult) -> None:
        """After the loop: ONE copy back of the scored plan's float64 blob (log-probabilities | no-speech probabilities)."""
        B, T, P, eos = pl["B"], self.geo.max_target_positions, pl["P"], pl["spec"].eos_token_id
        blob = pl["score_blob"].cpu().numpy()
        lp = blob[: B * T].reshape(B, T)
        res.no_speech_prob = blob[B * T:].copy()
        res.token_logprobs, res.avg_logprob = [], np.full(B, np.nan, dtype=np.float64)
        for b in range(B):
            gen = res.sequences[b, P:].tolist()
            n = gen.index(eos) + 1 if eos in gen else len(gen)                # the first eos included, nothing after it
            t = lp[b, P - 1: P - 1 + n].copy()                                # position p decides token p + 1
            res.token_logprobs.append(t)
            if n:
                total = 0.0
                for v in t:                                                   # ascending order, as a cumulative sum over one row
                    total += float(v)
                res.avg_logprob[b] = total / n

    def _generate_beams(self, enc_last, B: int, spec, language, slot: int, K: int, length_penalty: float, keep_logits: bool) -> DecodeResult:
        """The beam run: the prompt steps through ser_dec_select_v on all B K rows, then ser_beam_select_v as the last command of every
        step; the host reads the count of utterances not done every CHECK_EVERY steps, and one buffer after the loop."""
        pl = self.begin(B, spec, language, slot, num_beams=K, length_penalty=length_penalty)
        spec = pl["spec"]
        self.project_cross(pl, enc_last)
        n_max, forced, host, P = pl["n_max"], pl["forced_host"], pl["host"], spec.PROMPT_LEN
        V = self.geo.decoder_vocab_size
        kept = [] if keep_logits else None
        steps = 0
        for pos in range(n_max - 1):
            beam = pos >= P - 1
            self._run_step(pl, with_logits=forced[pos] < 0, beam=beam)
            steps += 1
            if beam and kept is not None:
                kept.append(pl["logits"][:, :V].clone())
            if beam and steps % self.CHECK_EVERY == 0:
                host[0:1].copy_(pl["unfinished"], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                if int(host[0]) == 0:
                    break
        return self._beam_result(pl, steps, kept)

    def _beam_result(self, pl, steps: int, kept) -> DecodeResult:
        from . import beam as BM
        spec, K, Bu, lay = pl["spec"], pl["K"], pl["Bu"], pl["beam_layout"]
        P = spec.PROMPT_LEN
        pl["beam_host"].copy_(pl["beam_blob"], non_blocking=True)
        head = pl["ids"][::K, :P].cpu().numpy().astype(np.int64)               # the prompt (rows of an utterance are identical there)
        margins = pl["margin"][::K, : P - 1].cpu().numpy()
        err = int(pl["err"].item()) & 0xffffffff
        bits = 0
        if pl["range_flag"] is not None:
            bits = int(pl["range_flag"].item())
            pl["range_flag"].zero_()
        torch.cuda.current_stream().synchronize()
        raw = pl["beam_host"].numpy()
        view = lambda name: raw[lay[name][0]: lay[name][0] + int(np.prod(lay[name][2])) * np.dtype(lay[name][1]).itemsize].view(lay[name][1]).reshape(lay[name][2]).copy()
        state, n = view("state"), steps + 1
        trace = dict(first=P - 1, run=view("trace_run")[:n], cand=view("trace_cand")[:n], cand_scores=view("cand_score")[:n],
                     fin_scores=view("fin_score"), fin_handles=view("fin_handle"), n_fin=state[:, 0].copy(), flags=state[:, 1].copy(),
                     done=state[:, 2].copy(), done_step=state[:, 3].copy(), run_scores=view("run"))
        failed = bool(bits & 1) or err != 0
        nbest = [[] for _ in range(Bu)]
        if not failed:
            nbest = BM.nbest(trace["run"], trace["cand"], trace["fin_scores"], trace["fin_handles"], trace["n_fin"], P - 1)
        rows = [nb[0][0] if nb else [] for nb in nbest]
        width = P + max([len(r) for r in rows] + [0])
        seqs = np.full((Bu, width), spec.pad_token_id, dtype=np.int64)
        seqs[:, :P] = head
        lists = []
        for b, r in enumerate(rows):
            seqs[b, P: P + len(r)] = r
            lists.append(r[: r.index(spec.eos_token_id)] if spec.eos_token_id in r else list(r))
        res = DecodeResult(seqs, head[:, 1].copy(), lists, margins, bits, err)
        res.nbest = nbest
        res.beam_scores = np.array([nb[0][1] if nb else np.nan for nb in nbest], dtype=np.float64)
        res.beam_trace, res.beam_gaps = trace, view("gaps")[:n]
        if kept is not None:
            res.beam_logits = torch.stack(kept) if kept else None
        return res

    def _ts_buffer(self, name: str, numel: int, dtype) -> torch.Tensor:
        """Grow-only storage of the timestamp stages, the decoder's (like the caches: no two batches are in flight)."""
        bufs = self.__dict__.setdefault("_ts_bufs", {})
        t = bufs.get(name)
        if t is None or t.numel() < numel:
            bufs[name] = None
            t = bufs[name] = torch.empty(numel, dtype=dtype, device=self.device)
        return t

    def _token_times(self, pl, res: DecodeResult, lengths: Sequence[int]) -> None:
        """After the loop: weights (ser_ts_weights_v), matrix (ser_ts_matrix_v) and DTW (ser_dtw_v) of the whole batch on the forward's
        stream, then ONE copy back: two status words and the first frames per utterance."""
        geo, spec, heads = self.geo, pl["spec"], pl["heads"]
        B, T, S, D, A = pl["B"], geo.max_target_positions, geo.max_source_positions, geo.hidden, len(heads)
        P = spec.PROMPT_LEN
        n_tok = []
        for b in range(B):
            gen = res.sequences[b, P:].tolist()
            n_tok.append(gen.index(spec.eos_token_id) + 1 if spec.eos_token_id in gen else len(gen))
        rows = [max(n - 1, 0) for n in n_tok]
        frames = [min((int(l) // 160) // 2, S) for l in lengths]
        R = max(1, max(rows))
        ld = (S + 3) // 4 * 4
        tab = pl["ts_tab"].begin()
        d_rows, d_frames = tab.put32(np.asarray(rows, dtype=np.int32)), tab.put32(np.asarray(frames, dtype=np.int32))
        tab.send()
        w = self._ts_buffer("w", B * A * R * ld, torch.float32)
        stats = self._ts_buffer("stats", B * A * S * 2, torch.float64)
        mat = self._ts_buffer("matrix", B * R * ld, torch.float32)
        work_bytes = int(lib.ser_dtw_work_bytes(B, R, S))
        work = self._ts_buffer("work", work_bytes // 8, torch.int64)
        out = pl["ts_out"]
        st = self._s()
        cross = pl["cross"]
        trace = getattr(self, "ts_trace", None)             # when a list: (stage, start event, end event) per stage (tools/whisper_timestamps_bench.py)

        def mark():
            if trace is None:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        t0 = mark()
        wa = _lib.TsWeightsArgs()
        wa.keep, wa.cross = pl["keep"].data_ptr(), cross.data_ptr()
        wa.layer_stride, wa.batch_stride, wa.ldc = cross.stride(0), S * 2 * D, 2 * D
        wa.n_rows, wa.n_frames, wa.w, wa.ld_w, wa.scale = d_rows.data_ptr(), d_frames.data_ptr(), w.data_ptr(), ld, 64 ** -0.5
        wa.B, wa.n_align, wa.n_keys, wa.pos0, wa.max_rows, wa.max_pos = B, A, S, P, R, T
        wa.n_layers, wa.H = geo.decoder_layers, geo.decoder_attention_heads
        for k, (l, h) in enumerate(heads):
            wa.head_layer[k], wa.head_index[k] = l, h
        check(lib.ser_ts_weights_v(C.byref(wa), st), "ser_ts_weights")
        t1 = mark()
        ma = _lib.TsMatrixArgs()
        ma.w, ma.ld_w, ma.n_rows, ma.n_frames, ma.stats = w.data_ptr(), ld, d_rows.data_ptr(), d_frames.data_ptr(), stats.data_ptr()
        ma.matrix, ma.ld_m, ma.status = mat.data_ptr(), ld, out.data_ptr()
        ma.B, ma.n_align, ma.max_rows, ma.max_frames, ma.width = B, A, R, S, int(spec.median_filter_width)
        check(lib.ser_ts_matrix_v(C.byref(ma), st), "ser_ts_matrix")
        t2 = mark()
        da = _lib.DtwArgs()
        da.matrix, da.ld_m, da.n_rows, da.n_frames = mat.data_ptr(), ld, d_rows.data_ptr(), d_frames.data_ptr()
        da.work, da.work_bytes = work.data_ptr(), work_bytes
        da.first_frame, da.ld_t, da.status = out.data_ptr() + 4 * 2 * B, T, out.data_ptr() + 4 * B
        da.B, da.max_rows, da.max_frames = B, R, S
        check(lib.ser_dtw_v(C.byref(da), st), "ser_dtw")
        if trace is not None:
            trace.extend((("weights", t0, t1), ("matrix", t1, t2), ("dtw", t2, mark())))
        host = pl["ts_host"]
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h = host.numpy()
        first = h[2 * B:].reshape(B, T)
        status = h[:B].copy()
        res.token_frames, res.token_times = [], []
        for b in range(B):
            if rows[b] >= 1 and frames[b] < 1:
                status[b] |= _lib.TS_NO_FRAMES
            if rows[b] >= 2:
                status[b] |= h[B + b]
            fr = first[b, : rows[b]].astype(np.int64)
            t = np.zeros(n_tok[b], dtype=np.float32)
            if rows[b] >= 1:
                t[: rows[b]] = (fr.astype(np.float64) * spec.TIME_PRECISION).astype(np.float32)
                t[rows[b]] = t[rows[b] - 1]
            res.token_frames.append(None if status[b] else fr)
            res.token_times.append(None if status[b] else t)
        res.ts_status = status
        res.ts_matrix = mat[: B * R * ld].view(B, R, ld)

    def result(self, pl, steps: int) -> DecodeResult:
        spec = pl["spec"]
        ids = pl["ids"][:, : steps + 1].cpu().numpy().astype(np.int64)
        margins = pl["margin"][:, :steps].cpu().numpy()
        err = int(pl["err"].item()) & 0xffffffff
        bits = 0
        if pl["range_flag"] is not None:
            bits = int(pl["range_flag"].item())
            pl["range_flag"].zero_()
        P = pl.get("P", spec.PROMPT_LEN)
        lists, ends = [], []
        for row in ids:
            gen = row[P:].tolist()
            cut = gen.index(spec.eos_token_id) if spec.eos_token_id in gen else None
            lists.append(gen if cut is None else gen[:cut])
            ends.append(ids.shape[1] if cut is None else P + cut + 1)
        n = max(ends)                                   # the length at which every row had finished (steps past it wrote pad only)
        return DecodeResult(ids[:, :n], ids[:, 1].copy(), lists, margins[:, : n - 1], bits, err)


class ProsodyFeatures(HiddenStates):
    """What ``ProsodyEncoder.forward`` returns: ``rows`` [M, D] fp32 (the tensor the reference saves per file, packed), ``codes`` [M]
    int32, ``gaps`` [M] fp32 (distance of the second-nearest code minus the nearest's) and ``z`` [M, D] (the encoder's last LayerNorm, the
    quantizer's input), all on the device and valid until the slot's next forward; utterance b owns rows frame_offs[b]:frame_offs[b + 1]
    with ``len_b // 200 + 1`` frames.  As ``HiddenStates`` it holds one state -- the rows -- so that a head reads them in place
    (``RowSource``).  ``err``: ser_fvq_v's error word (a latent that was not finite)."""

    def __init__(self, rows, codes, gaps, z, mel, frame_offs, range_flag, frame_offs_dev, err):
        super().__init__(rows.unsqueeze(0), frame_offs, range_flag=range_flag, frame_offs_dev=frame_offs_dev)
        self.rows, self.codes, self.gaps, self.z, self.mel, self.err = rows, codes, gaps, z, mel, err

    def take_range_bits(self, pinned_out: Optional[torch.Tensor] = None):
        """The guard bits of the forward, with bit 0 set as well when the quantizer's error word is: such a batch fails like a range-guard
        hit.  Synchronous (the error word is read back); both words are cleared."""
        bits = super().take_range_bits() | (1 if int(self.err.item()) else 0)
        self.err.zero_()
        if pinned_out is not None:
            pinned_out.fill_(bits)
            return None
        return bits


class _PreLnStack(_LaunchHost):
    """The pre-LayerNorm layers of src/ns3/transformer.py's TransformerEncoder (melspec_encoder, timbre_encoder) on libserhip:
    ser_layernorm_v, ser_gemm (FC1's k = 5 convolution as an implicit GEMM over a zero-halo'd copy), ser_attention_v and ser_act_rows_v
    for the ReLU.  ``pl``: the buffers of one slot -- xa, qkv, ctx, tmp, halo, f1, ffn, halo_rowmap, fc1_rowoff, frame_offs, B, M, Tmax."""

    def _act_rows(self, x: torch.Tensor, ldx: int, out: Act, rows: int, D: int, relu: bool, rowmap=None) -> None:
        a = self._cmd("act_rows")
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = x.data_ptr(), ldx, out.ptr, out.cols, out.plane_stride
        a.out_rowmap, a.range_flag = _ptr(rowmap), self._flag
        a.relu, a.mode, a.rows, a.D = int(relu), self.mode, rows, D
        self._issue(_lib.OP_ACT_ROWS, a, "ser_act_rows", rows=rows)

    def _attn(self, pl, sp=None) -> None:
        sp = self.spec if sp is None else sp
        qkv, out = pl["qkv"], pl["ctx"]
        a = self._cmd("attention")
        a.qkv, a.ld, a.plane_stride = qkv.ptr, qkv.cols, qkv.plane_stride
        a.q_col, a.k_col, a.v_col, a.B = 0, sp.hidden, 2 * sp.hidden, pl["B"]
        a.frame_offs, a.max_frames = pl["frame_offs"].data_ptr(), pl["Tmax"]
        a.out, a.ldo, a.out_plane_stride = out.ptr, out.cols, out.plane_stride
        a.H, a.dh, a.scale, a.mode = sp.heads, sp.head_dim, -1.0, self.mode          # q is pre-scaled
        self._issue(_lib.OP_ATTENTION, a, "ser_attention", B=pl["B"], max_frames=pl["Tmax"])

    def _pre_ln_layers(self, pl, sp, layers, x: torch.Tensor, h: torch.Tensor, x_in: Optional[torch.Tensor] = None) -> None:
        """the layers on the residual stream ``x`` (``h``: the stream between a layer's two halves); ``x_in``: where layer 0 reads its
        input when that is not ``x`` itself"""
        M, D, F = pl["M"], sp.hidden, sp.ffn
        scale = sp.head_dim ** -0.5 * 1.4426950408889634          # q leaves multiplied by dh^-0.5 * log2(e) (exp2-domain softmax)
        src = x if x_in is None else x_in
        for lay in layers:
            # x += MHA(LN1(x))
            self._layernorm(src, D, lay["ln1"], M, D, out_act=pl["xa"], eps=1e-5)
            self._gemm(pl["xa"], lay["qkv"], M, out_act=pl["qkv"], col_scale=scale, col_scale_end=D)
            self._attn(pl, sp)
            self._gemm(pl["ctx"], lay["out"], M, residual=src, ldr=D, out_f32=h, ldo_f32=D)
            # h += Linear(ReLU(Conv1d_k5(LN2(h)))): LN2's rows go to their halo'd positions, FC1 reads k consecutive rows per frame
            self._layernorm(h, D, lay["ln2"], M, D, out_f32=pl["tmp"], eps=1e-5)
            self._act_rows(pl["tmp"], D, pl["halo"], M, D, relu=False, rowmap=pl["halo_rowmap"])
            self._gemm(pl["halo"], lay["fc1"], M, a_rowoff=pl["fc1_rowoff"], out_f32=pl["f1"], ldo_f32=F)
            self._act_rows(pl["f1"], F, pl["ffn"], M, F, relu=True)
            self._gemm(pl["ffn"], lay["fc2"], M, residual=h, ldr=D, out_f32=x, ldo_f32=D)
            src = x

    def _upload_layers(self, layers, prefix: str) -> list:
        pair = lambda t: (self._dev_f32(t[0]), self._dev_f32(t[1]))
        out = []
        for i, lw in enumerate(layers):
            p = f"{prefix}.layers.{i}"
            out.append(dict(
                ln1=pair(lw["ln1"]), ln2=pair(lw["ln2"]),
                qkv=self._linear(*lw["qkv"], name=p + ".self_attn.in_proj_weight"), out=self._linear(*lw["out"], name=p + ".self_attn.out_proj.weight"),
                fc1=self._linear(*lw["fc1"], name=p + ".ffn.ffn_1.weight"), fc2=self._linear(*lw["fc2"], name=p + ".ffn.ffn_2.weight")))
        return out


class _ConformerLayers:
    """The conformer layer of ``W2vBertEncoder`` and ``ConformerSpeechEncoder`` (a mixin in front of ``_EncoderBase``):
        x += FFN1(LN x) / 2;  x += Attn(LN x);  x += Conv(..);  x += FFN2(LN x) / 2;  x = LN x
    on ser_layernorm_v and ser_gemm, with ser_swish_rows_v between a feed-forward block's GEMMs and ser_conformer_conv_v or
    ser_conformer_conv_bn_v between the convolution module's pointwise GEMMs.  The two 1/2 factors are folded into the blocks' output
    Linears at load.  An encoder adds its own front end, attention step (r1 -> ctx) and position weights, buffers and tables."""

    def _q_scale(self) -> float:
        """q leaves its projection multiplied by dh^-0.5 * log2(e) (exp2-domain softmax)"""
        return self.geo.head_dim ** -0.5 * 1.4426950408889634

    def _check_conformer_geometry(self, attention: str, distances: Optional[int] = None) -> None:
        geo = self.geo
        D, dh, K = geo.hidden, geo.head_dim, geo.conv_depthwise_kernel
        if dh != 64:
            raise ValueError(f"the {attention} attention is built for heads of 64 (hidden {D} / {geo.heads} heads = {dh})")
        if D % 64 or geo.ffn % 64 or D > 2048:
            raise ValueError(f"hidden {D} / intermediate {geo.ffn} must be multiples of 64, hidden <= 2048")
        if not (K & 1) or K > 31 or (distances is not None and distances > 128):
            tail = "" if distances is None else f" / {distances} distances (<= 128)"
            raise ValueError(f"depthwise kernel {K} (odd, <= 31){tail} unsupported")

    def _conformer_layer_weights(self, sd, i: int) -> dict:
        """what the families share of layer ``i``; the caller adds its attention projections, position weights and the conv module's norm
        (``dw_ln``: LayerNorm, or ``bn``: the folded BatchNorm)"""
        from .weights import fold_w2v_bert_ffn
        D, K = self.geo.hidden, self.geo.conv_depthwise_kernel
        p = f"encoder.layers.{i}"
        a, c = p + ".self_attn", p + ".conv_module"
        lay = {}
        for f in ("ffn1", "ffn2"):
            lay[f + "_ln"] = self._ln_pair(sd, f"{p}.{f}_layer_norm")
            lay[f + "_fc1"] = self._linear(sd[f"{p}.{f}.intermediate_dense.weight"], sd[f"{p}.{f}.intermediate_dense.bias"],
                                           name=f"{p}.{f}.intermediate_dense.weight")
            lay[f + "_fc2"] = self._linear(*fold_w2v_bert_ffn(sd[f"{p}.{f}.output_dense.weight"], sd[f"{p}.{f}.output_dense.bias"]),
                                           name=f"{p}.{f}.output_dense.weight")
        lay["attn_ln"] = self._ln_pair(sd, p + ".self_attn_layer_norm")
        lay["out"] = self._linear(sd[a + ".linear_out.weight"], sd[a + ".linear_out.bias"], name=a + ".linear_out.weight")
        lay["conv_ln"] = self._ln_pair(sd, c + ".layer_norm")
        lay["pw1"] = self._linear(sd[c + ".pointwise_conv1.weight"].reshape(2 * D, D), None, name=c + ".pointwise_conv1.weight")
        lay["dw"] = self._dev_f32(sd[c + ".depthwise_conv.weight"].reshape(D, K).t())        # [K][D]: a thread's 4 channels are one load
        lay["pw2"] = self._linear(sd[c + ".pointwise_conv2.weight"].reshape(D, D), None, name=c + ".pointwise_conv2.weight")
        lay["final_ln"] = self._ln_pair(sd, p + ".final_layer_norm")
        return lay

    def _conformer_buffers(self, ar: dict, M: int) -> None:
        geo, dev = self.geo, self.device
        D, F = geo.hidden, geo.ffn
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ar["states"] = f32(geo.num_layers + 1, M, D)
        ar["r1"], ar["r2"], ar["r3"], ar["r4"] = f32(M, D), f32(M, D), f32(M, D), f32(M, D)
        ar["f1"], ar["pw"] = f32(M, F), f32(M, 2 * D)
        ar["xa"], ar["ctx"], ar["cv"] = self._new_act(M, D), self._new_act(M, D), self._new_act(M, D)
        ar["qkv"], ar["ffn"] = self._new_act(M, 3 * D), self._new_act(M, F)

    def _swish_rows(self, x: torch.Tensor, out: Act, rows: int, D: int) -> None:
        a = self._cmd("swish_rows")
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = x.data_ptr(), D, out.ptr, out.cols, out.plane_stride
        a.range_flag, a.mode, a.rows, a.D = self._flag, self.mode, rows, D
        self._issue(_lib.OP_SWISH_ROWS, a, "ser_swish_rows", rows=rows)

    def _ffn_half(self, pl, lay, f: str, x: torch.Tensor, out: torch.Tensor, eps=None) -> None:
        """out = x + FFN(LN x) / 2 (the half sits in the output Linear); ``eps``: the LayerNorm's, default the geometry's"""
        M, D, F = pl["M"], self.geo.hidden, self.geo.ffn
        self._layernorm(x, D, lay[f + "_ln"], M, D, out_act=pl["xa"], eps=eps)
        self._gemm(pl["xa"], lay[f + "_fc1"], M, out_f32=pl["f1"], ldo_f32=F)
        self._swish_rows(pl["f1"], pl["ffn"], M, F)
        self._gemm(pl["ffn"], lay[f + "_fc2"], M, residual=x, ldr=D, out_f32=out, ldo_f32=D)

    def _conv_mid(self, pl, lay) -> None:
        """pw -> cv through the norm the layer carries: ``bn`` (centred window, ser_conformer_conv_bn_v) or ``dw_ln`` (causal window)"""
        geo, out, bn = self.geo, pl["cv"], "bn" in lay
        a = self._cmd("conformer_conv_bn" if bn else "conformer_conv")
        a.y, a.ldy, a.w = pl["pw"].data_ptr(), 2 * geo.hidden, lay["dw"].data_ptr()
        if bn:
            a.scale, a.shift = lay["bn"][0].data_ptr(), lay["bn"][1].data_ptr()
        else:
            a.gamma, a.beta, a.eps = lay["dw_ln"][0].data_ptr(), lay["dw_ln"][1].data_ptr(), float(geo.layer_norm_eps)
        a.frame_offs, a.out_act, a.ldo_act, a.out_plane_stride = pl["frame_offs"].data_ptr(), out.ptr, out.cols, out.plane_stride
        a.range_flag = self._flag
        a.B, a.D, a.K, a.max_frames, a.rows, a.mode = pl["B"], geo.hidden, geo.conv_depthwise_kernel, pl["Tmax"], pl["M"], self.mode
        self._issue(_lib.OP_CONFORMER_CONV_BN if bn else _lib.OP_CONFORMER_CONV, a, "ser_conformer_conv_bn" if bn else "ser_conformer_conv",
                    B=pl["B"], max_frames=pl["Tmax"], rows=pl["M"])

    def _biased_attention_cmd(self, pl, field: str):
        """an ``attention_rk`` / ``attention_rb`` command over the packed q | k | v with its embedded ``base`` filled; the caller sets the bias
        fields and issues it"""
        geo = self.geo
        D, qkv, out = geo.hidden, pl["qkv"], pl["ctx"]
        r = self._cmd(field)
        a = r.base
        a.qkv, a.ld, a.plane_stride = qkv.ptr, qkv.cols, qkv.plane_stride
        a.q_col, a.k_col, a.v_col, a.B = 0, D, 2 * D, pl["B"]
        a.frame_offs, a.max_frames = pl["frame_offs"].data_ptr(), pl["Tmax"]
        a.out, a.ldo, a.out_plane_stride = out.ptr, out.cols, out.plane_stride
        a.H, a.dh, a.scale, a.mode = geo.heads, geo.head_dim, -1.0, self.mode          # q is pre-scaled
        if self._rec is not None:                                               # the per-batch sizes live in the embedded base struct
            self._rec.patches += [(a, "B", "B"), (a, "max_frames", "Tmax")]
        return r

    def _conformer_layers(self, pl, attention, last_state: Optional[int], eps=None, enc_ln=None) -> None:
        """the layers from states[0] on.  ``attention(pl, lay, scale)``: the encoder's step from r1 to ctx, the layer's attention LayerNorm
        included; ``eps``: the layers' LayerNorm eps (None: the geometry's); ``enc_ln``: a LayerNorm over the last layer's output, which
        then goes through ``last`` (None: every layer writes its state directly)"""
        geo = self.geo
        M, D, L = pl["M"], geo.hidden, geo.num_layers
        states, scale = pl["states"], self._q_scale()
        for i, lay in enumerate(self.layers):
            via_last = enc_ln is not None and i + 1 == L
            self._ffn_half(pl, lay, "ffn1", states[i], pl["r1"], eps=eps)
            attention(pl, lay, scale)
            self._gemm(pl["ctx"], lay["out"], M, residual=pl["r1"], ldr=D, out_f32=pl["r2"], ldo_f32=D)
            self._layernorm(pl["r2"], D, lay["conv_ln"], M, D, out_act=pl["xa"], eps=eps)
            self._gemm(pl["xa"], lay["pw1"], M, out_f32=pl["pw"], ldo_f32=2 * D)
            self._conv_mid(pl, lay)
            self._gemm(pl["cv"], lay["pw2"], M, residual=pl["r2"], ldr=D, out_f32=pl["r3"], ldo_f32=D)
            self._ffn_half(pl, lay, "ffn2", pl["r3"], pl["r4"], eps=eps)
            self._layernorm(pl["r4"], D, lay["final_ln"], M, D, out_f32=pl["last"] if via_last else states[i + 1], eps=eps)
            if via_last:
                self._layernorm(pl["last"], D, enc_ln, M, D, out_f32=states[L])
            if self._state_done(i + 1, last_state):
                return


class ProsodyEncoder(_WaveIO, _PreLnStack):
    """The prosody stream of the reference's three-stream heads (preprocessing/preprocess_ns3_prosody.py) on libserhip: NS3 log-mel +
    melspec_linear (ser_prosody_mel_v), melspec_encoder's pre-LayerNorm layers -- ser_layernorm_v, ser_gemm (FC1's k = 5 convolution as an
    implicit GEMM over a zero-halo'd copy, two zero rows around each utterance), ser_attention_v, ser_act_rows_v for the ReLU -- and the
    first quantizer's lookup (ser_fvq_v).  ``state_dict``: ns3_facodec_decoder_v2.bin's (``prosody.load_state_dict``); geometry from its
    shapes, ``heads`` is not in them.  Every utterance alone, as the reference's batch of one; 16 kHz input of at least 400 samples."""

    def __init__(self, state_dict, device="cuda:0", mode: str = "f16x", heads: int = 4):
        from . import prosody as P
        from .frontend import prosody_dft_table, prosody_mel_filters
        if mode not in POST_LN_MODES:
            raise ValueError(f"the prosody encoder supports the {', '.join(POST_LN_MODES)} numerics modes")
        fp16_planes = mode == "f16x" and _os.environ.get("SER_NO_RANGE_GUARD", "0") != "1"
        super().__init__(device, mode, MODES[mode], MODES[mode], fp16_planes)
        w = P.prepare(state_dict, heads)
        self.spec = spec = w["spec"]
        melw = prosody_mel_filters(spec.n_mels)
        self.n_bins = int(melw.shape[1])
        self.melw = self._dev_f32(torch.from_numpy(melw))
        self.dft = torch.from_numpy(prosody_dft_table(self.n_bins)).to(self.device)
        self.lin_w, self.lin_b = self._dev_f32(w["lin_w"]), self._dev_f32(w["lin_b"])
        self.layers = self._upload_layers(w["layers"], P.ENC)
        self.last_ln = (self._dev_f32(w["last_ln"][0]), self._dev_f32(w["last_ln"][1]))
        self.w_in, self.b_in = self._dev_f32(w["w_in"]), self._dev_f32(w["b_in"])
        self.codes, self.table = self._dev_f32(w["codes"]), self._dev_f32(w["table"])
        self._arenas = SlotArenas(self._build_arena)

    # ------------------------------------------------------------------ buffers
    def _build_arena(self, cap: Dict[str, int]) -> dict:
        """buffer set of one slot (pointers fixed between batches: the command list is recorded once per arena)"""
        M, B, sp, dev = cap["M"], cap["B"], self.spec, self.device
        D, F = sp.hidden, sp.ffn
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ar = {}
        ar["x"], ar["h"], ar["tmp"], ar["z"], ar["rows"] = f32(M, D), f32(M, D), f32(M, D), f32(M, D), f32(M, D)
        ar["f1"], ar["mel"], ar["gaps"] = f32(M, F), f32(M, sp.n_mels), f32(M)
        ar["codes"] = torch.empty(M, dtype=torch.int32, device=dev)
        ar["xa"], ar["ctx"], ar["qkv"], ar["ffn"] = self._new_act(M, D), self._new_act(M, D), self._new_act(M, 3 * D), self._new_act(M, F)
        ar["halo"] = self._new_act(M + (sp.kernel // 2) * (B + 1), D, zero=True)
        ar["halo_rowmap"] = torch.empty(M, dtype=torch.int32, device=dev)
        ar["fc1_rowoff"] = torch.empty(M, dtype=torch.int32, device=dev)
        ar["tab"] = TableBlob(B, 4, dev)                        # sample_offs | frame_offs (int32) | halo base | FC1 tap base
        ar["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.fp16_planes:
            ar["range_flag"] = torch.zeros(1, dtype=torch.int32, device=dev)
        return ar

    def _plan(self, lengths: Sequence[int], slot: int = 0) -> dict:
        from .frontend import PROSODY_MIN_SAMPLES, prosody_frames
        lengths = tuple(int(n) for n in lengths)
        B = len(lengths)
        if B == 0 or min(lengths) < PROSODY_MIN_SAMPLES:
            raise ValueError(f"utterance shorter than {PROSODY_MIN_SAMPLES} samples: it cannot be reflect-padded (the reference fails such a file)")
        T = [prosody_frames(n) for n in lengths]
        offs = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
        M, Tmax, half = int(offs[-1]), max(T), self.spec.kernel // 2
        ar = self._arenas.fit(slot, M=M, B=B)
        if ar["plan"] is not None and ar["plan"]["lengths"] == lengths:
            return ar["plan"]
        tab = ar["tab"].begin()
        so, fo = tab.put64(np.concatenate([[0], np.cumsum(lengths)])), tab.put32(offs)
        _, halo_index = _halo_layout(tab, offs, fo, half, self.spec.hidden, ar["halo_rowmap"], [ar["fc1_rowoff"]], ar["halo"])
        tab.send()
        halo_index(_stream(), ar["plan"] is not None)
        pl = dict(ar)
        pl.update(lengths=lengths, B=Sz(B, "B"), M=Sz(M, "M"), Tmax=Sz(Tmax, "Tmax"), sizes=dict(B=B, M=M, Tmax=Tmax),
                  sample_offs=so, frame_offs=fo, frame_offs_host=[int(v) for v in offs])
        ar["plan"] = pl
        return pl

    # ------------------------------------------------------------------ launches
    def _mel(self, pl, packed_wave: torch.Tensor, with_linear: bool = True) -> None:
        sp = self.spec
        a = self._cmd("prosody_mel")
        a.wav, a.sample_offs, a.frame_offs = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["frame_offs"].data_ptr()
        a.dft, a.mel, a.mel_out = self.dft.data_ptr(), self.melw.data_ptr(), pl["mel"].data_ptr()
        if with_linear:
            a.lin_w, a.lin_b, a.out, a.ldo, a.D = self.lin_w.data_ptr(), self.lin_b.data_ptr(), pl["x"].data_ptr(), sp.hidden, sp.hidden
        a.B, a.max_frames, a.n_bins, a.n_mels = pl["B"], pl["Tmax"], self.n_bins, sp.n_mels
        self._issue(_lib.OP_PROSODY_MEL, a, "ser_prosody_mel", input="wav", B=pl["B"], max_frames=pl["Tmax"])

    def _fvq(self, pl) -> None:
        sp = self.spec
        a = self._cmd("fvq")
        a.z, a.ldz, a.w_in, a.b_in, a.codes = pl["z"].data_ptr(), sp.hidden, self.w_in.data_ptr(), self.b_in.data_ptr(), self.codes.data_ptr()
        a.table, a.ld_table, a.idx, a.gap = self.table.data_ptr(), sp.hidden, pl["codes"].data_ptr(), pl["gaps"].data_ptr()
        a.out_f32, a.ldo_f32, a.err = pl["rows"].data_ptr(), pl.get("rows_ld", sp.hidden), pl["err"].data_ptr()   # rows_ld: a column block of a wider buffer
        a.rows, a.D, a.n_codes, a.code_dim, a.mode = pl["M"], sp.hidden, sp.n_codes, sp.code_dim, self.mode
        self._issue(_lib.OP_FVQ, a, "ser_fvq", rows=pl["M"])

    def _launches(self, pl, packed_wave: torch.Tensor, last_state: Optional[int] = None) -> None:
        sp = self.spec
        M, D = pl["M"], sp.hidden
        x = pl["x"]
        self._mel(pl, packed_wave)
        self._pre_ln_layers(pl, sp, self.layers, x, pl["h"])
        self._layernorm(x, D, self.last_ln, M, D, out_f32=pl["z"], eps=1e-5)
        self._fvq(pl)

    def _result(self, pl, flag) -> ProsodyFeatures:
        M = int(pl["M"])
        return ProsodyFeatures(pl["rows"][:M], pl["codes"][:M], pl["gaps"][:M], pl["z"][:M], pl["mel"][:M], pl["frame_offs_host"], flag,
                               pl["frame_offs"], pl["err"])

    def _ingest(self, waves, lengths, slot: int):
        """(plan, packed samples on the device) of a list of raw waveforms, or of samples the caller packed (``lengths`` given)"""
        if lengths is not None:
            return self._plan(lengths, slot), waves
        waves = [np.ascontiguousarray(w, dtype=np.float32) for w in waves]
        pl = self._plan([len(w) for w in waves], slot)                # refuses a short wave before anything is uploaded
        return pl, self.upload(waves, slot)

    @_on_stream
    def forward(self, waves, lengths: Optional[Sequence[int]] = None, slot: int = 0) -> ProsodyFeatures:
        """``waves``: a list of raw 16 kHz fp32 waveforms (uploaded here), or with ``lengths`` their packed samples on the device."""
        pl, waves = self._ingest(waves, lengths, slot)
        flag = pl.get("range_flag")
        self._flag = None if flag is None else flag.data_ptr()
        self._replay((self._arenas[slot],), pl["sizes"], lambda last: self._launches(pl, waves), waves.data_ptr())
        return self._result(pl, flag)

    @_on_stream
    def log_mel(self, waves, lengths: Optional[Sequence[int]] = None, slot: int = 0) -> torch.Tensor:
        """the [M, 20] log-mel rows alone (ser_prosody_mel_v without melspec_linear)"""
        pl, waves = self._ingest(waves, lengths, slot)
        self._mel(pl, waves, with_linear=False)
        return pl["mel"][: int(pl["M"])]


class SpeakerProsodyFeatures(ProsodyFeatures):
    """``ProsodyFeatures`` of the 512-wide stream: ``rows`` [M, 2 D] = prosody rows | timbre rows (what the reference saves per file,
    packed); ``encoded`` [M, D] = the codec encoder's output (the timbre layers' input without the position-0 vector the final
    convolution's bias carries: one fp32 subtraction, made when asked)."""

    def __init__(self, rows, codes, gaps, z, mel, frame_offs, range_flag, frame_offs_dev, err, enc_x, pos0, levels=None):
        super().__init__(rows, codes, gaps, z, mel, frame_offs, range_flag, frame_offs_dev, err)
        self._enc_x, self._pos0, self.levels = enc_x, pos0, levels

    @property
    def encoded(self) -> torch.Tensor:
        return self._enc_x - self._pos0


class SpeakerProsodyEncoder(_WaveIO, _PreLnStack):
    """The reference's 512-wide third stream (preprocessing/preprocess_ns3_prosody_speaker.py) on libserhip: a ``ProsodyEncoder`` for the
    first half and, for the second, FACodecEncoderV2.block -- narrow levels (C <= 32) on ser_codec_conv_v / ser_codec_unit_v, wide ones
    (C % 64 == 0) on ser_snake_v + ser_gemm over a zero-halo'd operand copy (27 zero rows around each utterance) -- followed by
    FACodecDecoderV2.timbre_encoder's pre-LayerNorm layers, all on one stream and one command list.  ser_fvq_v writes columns 0:D and the
    timbre encoder's last LayerNorm columns D:2D of one [M, 2 D] buffer.  ``decoder_sd`` / ``encoder_sd``: the state dicts of
    ns3_facodec_decoder_v2.bin / ns3_facodec_encoder_v2.bin; 16 kHz input of at least 400 samples, every utterance alone."""

    def __init__(self, decoder_sd, encoder_sd, device="cuda:0", mode: str = "f16x", heads: int = 4):
        from . import prosody as P
        if mode not in POST_LN_MODES:
            raise ValueError(f"the prosody encoders support the {', '.join(POST_LN_MODES)} numerics modes")
        w = P.prepare_codec(encoder_sd, decoder_sd, heads)               # refuses an unsupported geometry before anything is uploaded
        self.prosody = ProsodyEncoder(decoder_sd, device, mode, heads)
        if self.prosody.spec.hidden != w["spec"].out_channels:
            raise ValueError(f"prosody rows are {self.prosody.spec.hidden} wide, timbre rows {w['spec'].out_channels}: not the halves of one tensor")
        super().__init__(device, mode, MODES[mode], MODES[mode], self.prosody.fp16_planes)
        self.spec = spec = w["spec"]
        dev = self._dev_f32
        kmajor = lambda t: dev(t.t().contiguous())                       # the narrow kernels read [k C_in][C_out]
        act = lambda a: (dev(a[0]), dev(a[1]))
        self.taps = dev(w["taps"])
        self.conv_in = (kmajor(w["conv_in"][0]), dev(w["conv_in"][1]))
        self.levels = []
        for i, lv in enumerate(w["levels"], start=1):
            narrow = lv["C"] <= P.NARROW_MAX
            units = []
            for j, u in enumerate(lv["units"]):
                p = f"block.{i}.block.{j}.block"
                if narrow:
                    units.append(dict(d=u["d"], act1=act(u["act1"]), act2=act(u["act2"]), w7=kmajor(u["w7"]), b7=dev(u["b7"]),
                                      w1=kmajor(u["w1"]), b1=dev(u["b1"])))
                else:
                    units.append(dict(d=u["d"], act1=act(u["act1"]), act2=act(u["act2"]), w7=self._linear(u["w7"], u["b7"], name=p + ".1.weight"),
                                      w1=self._linear(u["w1"], u["b1"], name=p + ".3.weight")))
            down = (kmajor(lv["down"][0]), dev(lv["down"][1])) if narrow else self._linear(*lv["down"], name=f"block.{i}.block.4.weight")
            self.levels.append(dict(C=lv["C"], narrow=narrow, stride=lv["stride"], pad=lv["pad"], units=units, act=act(lv["act"]), down=down))
        n = len(spec.strides)
        self.final = dict(act=act(w["final"]["act"]), lin=self._linear(w["final"]["w"], w["final"]["b"], name=f"block.{n + 2}.weight"))
        self.layers = self._upload_layers(w["layers"], P.TIMBRE)
        self.last_ln = (dev(w["last_ln"][0]), dev(w["last_ln"][1]))
        self.pos0 = dev(P.position0(spec.out_channels).float())
        self.halo = P.WIDE_HALO
        self._arenas = SlotArenas(self._build_arena)

    # ------------------------------------------------------------------ buffers
    def _build_arena(self, cap: Dict[str, int]) -> dict:
        """buffer set of one slot, sized by the rows of level 0 (every other level's rows are its exact quotients)"""
        B, sp, dev = cap["B"], self.spec, self.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        ar = dict(lv=[])
        rows = cap["M0"]
        for l, C in enumerate(sp.channels):
            last = l == len(sp.strides)
            lv = dict(cap=rows, xa=f32(rows, C))
            if not last:
                lv["xb"] = f32(rows, C)
            if C > 32:                                                   # a wide level: operand copies for ser_gemm
                lv["halo"] = self._new_act(rows + self.halo * (B + 1), C, zero=True)
                lv["rowmap"] = i32(rows)
                if last:
                    lv["rowoff_k3"] = i32(rows)
                else:
                    lv["h"], lv["a2"] = f32(rows, C), self._new_act(rows, C)
                    lv["rowoff"] = i32(3, rows)
                    lv["down_rowoff"] = i32(rows // sp.strides[l])
            ar["lv"].append(lv)
            if not last:
                rows //= sp.strides[l]
        M, ts = rows, sp.timbre
        D, F = ts.hidden, ts.ffn
        ar["enc"], ar["x"], ar["h"], ar["tmp"], ar["f1"], ar["rows2"] = f32(M, D), f32(M, D), f32(M, D), f32(M, D), f32(M, F), f32(M, 2 * D)
        ar["xa"], ar["ctx"], ar["qkv"], ar["ffn"] = self._new_act(M, D), self._new_act(M, D), self._new_act(M, 3 * D), self._new_act(M, F)
        ar["halo"] = self._new_act(M + (ts.kernel // 2) * (B + 1), D, zero=True)
        ar["halo_rowmap"], ar["fc1_rowoff"] = i32(M), i32(M)
        # per level offs (int32) and offs64; a wide level's halo base and tap bases (3 + the downsampling's, or 1); the timbre layers' two
        ar["tab"] = TableBlob(B, sum(2 + (0 if C <= 32 else 2 if l == len(sp.strides) else 5) for l, C in enumerate(sp.channels)) + 2, dev)
        return ar

    def _plan(self, lengths: Sequence[int], slot: int = 0) -> dict:
        ppl = self.prosody._plan(lengths, slot)                          # refuses a short wave before anything is uploaded
        lengths, B, sp = ppl["lengths"], int(ppl["B"]), self.spec
        lens = np.array([sp.level_lengths(n) for n in lengths], dtype=np.int64)        # [B, levels]
        offs = np.concatenate([np.zeros((1, lens.shape[1]), dtype=np.int64), np.cumsum(lens, axis=0)]).T   # [levels, B + 1]
        ar = self._arenas.fit(slot, M0=int(offs[0, -1]), B=B)
        old = ar["plan"]
        if old is not None and old["ppl"] is ppl:
            return old
        assert int(offs[-1, -1]) == int(ppl["M"]) and lens[:, -1].tolist() == np.diff(ppl["frame_offs_host"]).tolist()
        st, ts, tab = _stream(), sp.timbre, ar["tab"].begin()
        for l, lv in enumerate(ar["lv"]):
            lv["offs"], lv["offs64"] = tab.put32(offs[l]), tab.put64(offs[l])
        index, downs = [], []
        for l, lv in enumerate(ar["lv"]):
            if "halo" not in lv:
                continue
            # a wide level's halo'd copy: the dilated k = 7 convolutions start 3 d rows earlier, the last level's k = 3 one row earlier
            wide = "rowoff" in lv
            starts, ix = _halo_layout(tab, offs[l], lv["offs"], self.halo, sp.channels[l], lv["rowmap"],
                                      lv["rowoff"] if wide else [lv["rowoff_k3"]], lv["halo"], taps=(3, 9, 27) if wide else (1,))
            index.append(ix)
            if wide:                                                     # the strided convolution into the next level: that level's rows
                downs.append((l, tab.put64(starts - self.levels[l]["pad"])))
        index.append(_halo_layout(tab, ppl["frame_offs_host"], ppl["frame_offs"], ts.kernel // 2, ts.hidden, ar["halo_rowmap"],
                                  [ar["fc1_rowoff"]], ar["halo"])[1])
        tab.send()
        for ix in index:
            ix(st, old is not None)
        for l, base in downs:
            check(lib.ser_ragged_index(ar["lv"][l + 1]["offs"].data_ptr(), base.data_ptr(), B, sp.strides[l], sp.channels[l], 8,
                                       ar["lv"][l]["down_rowoff"].data_ptr(), int(offs[l + 1, -1]), st), "ser_ragged_index")
        pl = dict(ar)
        sizes = dict(ppl["sizes"])
        for l in range(len(sp.channels)):
            sizes[f"M{l}"], sizes[f"R{l}"] = int(offs[l, -1]), int(lens[:, l].max())
        pp = dict(ppl)
        pp["rows"], pp["rows_ld"] = ar["rows2"], 2 * ts.hidden           # ser_fvq_v writes the left half of the saved rows
        pl.update(ppl=ppl, pp=pp, lengths=lengths, B=ppl["B"], M=ppl["M"], Tmax=ppl["Tmax"], frame_offs=ppl["frame_offs"], sizes=sizes,
                  Ms=[Sz(sizes[f"M{l}"], f"M{l}") for l in range(len(sp.channels))],
                  Rs=[Sz(sizes[f"R{l}"], f"R{l}") for l in range(len(sp.channels))])
        ar["plan"] = pl
        return pl

    # ------------------------------------------------------------------ launches
    def _unit(self, x, y, C: int, u, offs, B, rmax, rows) -> None:
        a = self._cmd("codec_unit")
        a.x, a.y, a.row_offs, a.taps = x.data_ptr(), y.data_ptr(), offs.data_ptr(), self.taps.data_ptr()
        a.ea1, a.ib1, a.ea2, a.ib2 = u["act1"][0].data_ptr(), u["act1"][1].data_ptr(), u["act2"][0].data_ptr(), u["act2"][1].data_ptr()
        a.w7, a.b7, a.w1, a.b1 = u["w7"].data_ptr(), u["b7"].data_ptr(), u["w1"].data_ptr(), u["b1"].data_ptr()
        a.B, a.C, a.k, a.dilation, a.max_rows, a.rows = B, C, 7, u["d"], rmax, rows
        self._issue(_lib.OP_CODEC_UNIT, a, "ser_codec_unit", B=B, max_rows=rmax, rows=rows)

    def _conv(self, x, in_offs, out_offs, act, wb, y, C_in: int, C_out: int, k: int, stride: int, pad: int, B, rmax, rows, input=None) -> None:
        a = self._cmd("codec_conv")
        a.x, a.in_offs, a.out_offs = x.data_ptr(), in_offs.data_ptr(), out_offs.data_ptr()
        if act is not None:
            a.taps, a.ea, a.ib = self.taps.data_ptr(), act[0].data_ptr(), act[1].data_ptr()
        a.w, a.bias, a.y, a.ldy = wb[0].data_ptr(), wb[1].data_ptr(), y.data_ptr(), C_out
        a.B, a.C_in, a.C_out, a.k, a.stride, a.pad, a.max_out_rows, a.rows = B, C_in, C_out, k, stride, pad, rmax, rows
        self._issue(_lib.OP_CODEC_CONV, a, "ser_codec_conv", input=input, B=B, max_out_rows=rmax, rows=rows)

    def _snake(self, x, C: int, act, offs, out: Act, rowmap, B, rmax, rows) -> None:
        a = self._cmd("snake")
        a.x, a.ldx, a.row_offs, a.taps, a.ea, a.ib = x.data_ptr(), C, offs.data_ptr(), self.taps.data_ptr(), act[0].data_ptr(), act[1].data_ptr()
        a.out_act, a.ldo_act, a.out_plane_stride, a.out_rowmap = out.ptr, out.cols, out.plane_stride, _ptr(rowmap)
        a.range_flag = self._flag
        a.B, a.C, a.max_rows, a.rows, a.mode = B, C, rmax, rows, self.mode
        self._issue(_lib.OP_SNAKE, a, "ser_snake", B=B, max_rows=rmax, rows=rows)

    def _keep_level(self, keep, name: str, x: torch.Tensor, rows) -> None:
        """a test's copy of a level's output; when recording, where the level's commands end (tools/codec_bench.py times the parts)"""
        if keep is not None:
            keep[name] = x[: int(rows)].clone()
        if self._rec is not None and not name.startswith("u"):
            self._rec.parts.append((name, self._rec.n))

    def _codec_launches(self, pl, packed_wave: torch.Tensor, keep: Optional[dict] = None) -> None:
        sp, B, Ms, Rs, lvs = self.spec, pl["B"], pl["Ms"], pl["Rs"], pl["lv"]
        x = lvs[0]["xa"]
        self._conv(packed_wave, pl["ppl"]["sample_offs"], lvs[0]["offs"], None, self.conv_in, x, 1, sp.ngf, 7, 1, 3, B, Rs[0], Ms[0], input="x")
        self._keep_level(keep, "conv_in", x, Ms[0])
        for l, L in enumerate(self.levels):
            lv, nxt, C, s = lvs[l], lvs[l + 1], L["C"], L["stride"]
            y = lv["xb"]
            for j, u in enumerate(L["units"]):
                if L["narrow"]:
                    self._unit(x, y, C, u, lv["offs"], B, Rs[l], Ms[l])
                else:
                    self._snake(x, C, u["act1"], lv["offs"], lv["halo"], lv["rowmap"], B, Rs[l], Ms[l])
                    self._gemm(lv["halo"], u["w7"], Ms[l], a_rowoff=lv["rowoff"][j], kc=C, ldj=u["d"] * C, out_f32=lv["h"], ldo_f32=C)
                    self._snake(lv["h"], C, u["act2"], lv["offs"], lv["a2"], None, B, Rs[l], Ms[l])
                    self._gemm(lv["a2"], u["w1"], Ms[l], residual=x, ldr=C, out_f32=y, ldo_f32=C)
                x, y = y, x
                self._keep_level(keep, f"u{l + 1}_{j}", x, Ms[l])
            if L["narrow"]:
                self._conv(x, lv["offs64"], nxt["offs"], L["act"], L["down"], nxt["xa"], C, 2 * C, 2 * s, s, L["pad"], B, Rs[l + 1], Ms[l + 1])
            else:
                self._snake(x, C, L["act"], lv["offs"], lv["halo"], lv["rowmap"], B, Rs[l], Ms[l])
                self._gemm(lv["halo"], L["down"], Ms[l + 1], a_rowoff=lv["down_rowoff"], out_f32=nxt["xa"], ldo_f32=2 * C)
            x = nxt["xa"]
            self._keep_level(keep, f"level_{l + 1}", x, Ms[l + 1])
        n = len(self.levels)
        lv, C, ts = lvs[n], sp.channels[n], sp.timbre
        D, M = ts.hidden, pl["M"]
        self._snake(x, C, self.final["act"], lv["offs"], lv["halo"], lv["rowmap"], B, Rs[n], Ms[n])
        self._gemm(lv["halo"], self.final["lin"], Ms[n], a_rowoff=lv["rowoff_k3"], out_f32=pl["enc"], ldo_f32=D)
        # the timbre encoder: its input is the codec's output plus the position-0 vector (in the final convolution's bias)
        self._pre_ln_layers(pl, ts, self.layers, pl["x"], pl["h"], x_in=pl["enc"])
        self._layernorm(pl["x"], D, self.last_ln, M, D, out_f32=pl["rows2"][:, D:], ldo_f32=2 * D, eps=1e-5)

    def _launch_all(self, pl, packed_wave: torch.Tensor, keep: Optional[dict] = None) -> None:
        self.prosody._launches(pl["pp"], packed_wave)
        self._keep_level(None, "prosody", packed_wave, 0)
        self._codec_launches(pl, packed_wave, keep)

    @_on_stream
    def forward(self, waves, lengths: Optional[Sequence[int]] = None, slot: int = 0, keep_levels: bool = False) -> SpeakerProsodyFeatures:
        """``waves``: a list of raw 16 kHz fp32 waveforms (uploaded here), or with ``lengths`` their packed samples on the device.
        ``keep_levels`` (tests): launch one by one and keep a copy of conv_in's, every unit's and every level's output in ``.levels``."""
        if lengths is None:
            waves = [np.ascontiguousarray(w, dtype=np.float32) for w in waves]
            pl = self._plan([len(w) for w in waves], slot)
            waves = self.upload(waves, slot)
        else:
            pl = self._plan(lengths, slot)
        pro = self.prosody
        flag = pl["ppl"].get("range_flag")
        self._flag = None if flag is None else flag.data_ptr()
        keep = {} if keep_levels else None
        if keep_levels:
            with self._launching(None, (pro,)):
                self._launch_all(pl, waves, keep)
        else:
            # the list points into the prosody encoder's arena as well: recorded again when either arena was replaced
            self._replay((self._arenas[slot], pro._arenas[slot]), pl["sizes"], lambda last: self._launch_all(pl, waves), waves.data_ptr(),
                         hosts=(pro,))
        M, pp = int(pl["M"]), pl["pp"]
        return SpeakerProsodyFeatures(pl["rows2"][:M], pp["codes"][:M], pp["gaps"][:M], pp["z"][:M], pp["mel"][:M], pp["frame_offs_host"], flag,
                                      pp["frame_offs"], pp["err"], pl["enc"][:M], self.pos0, keep)


class W2vBertEncoder(_ConformerLayers, _WaveIO, _EncoderBase):
    """w2v-BERT 2.0 (HF Wav2Vec2BertModel behind SeamlessM4TFeatureExtractor; not in the reference, whose heads take any [T, D] stream) on
    libserhip: the Kaldi fbank front end (ser_fbank_v), the feature projection, and ``_ConformerLayers``' layer
        x += FFN1(LN x) / 2;  x += Attn(LN x);  x += Conv(LN x);  x += FFN2(LN x) / 2;  x = LN x
    with ser_relkey_table_v + ser_attention_rk_v for the relative-key attention and ser_conformer_conv_v (causal window, LayerNorm) in the
    convolution module.  Every utterance alone: ``frames(n) = (1 + (n - 400) // 160) // stride`` rows, at least one."""

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "f16x"):
        from .frontend import w2vbert_dft_table, w2vbert_mel_filters
        super().__init__(geo, device, mode, post_ln=True)
        sd = state_dict
        D = geo.hidden
        self._check_conformer_geometry("relative-key", geo.distance_positions)
        melw, rng = w2vbert_mel_filters(geo.fbank_mels)
        self.melw = torch.from_numpy(melw).to(self.device)
        self.mel_range = torch.from_numpy(rng).to(self.device)
        self.dft = torch.from_numpy(w2vbert_dft_table()).to(self.device)
        # feature projection: LayerNorm(160) -> Linear(160 -> D); K is padded with zero columns to the GEMM's 64-deep tiles
        self.fdim = geo.fbank_dim
        self.fpad = ((self.fdim + 63) // 64) * 64
        self.proj_ln = self._ln_pair(sd, "feature_projection.layer_norm")
        w = torch.zeros(D, self.fpad)
        w[:, : self.fdim] = sd["feature_projection.projection.weight"].detach().float().cpu()
        self.proj = self._linear(w, sd["feature_projection.projection.bias"], name="feature_projection.projection.weight")
        self.qe_ld = ((geo.distance_positions + 3) // 4) * 4
        self.layers = []
        for i in range(geo.num_layers):
            a, c = f"encoder.layers.{i}.self_attn", f"encoder.layers.{i}.conv_module"
            lay = self._conformer_layer_weights(sd, i)
            lay["qkv"] = self._linear(torch.cat([sd[f"{a}.linear_{n}.weight"] for n in "qkv"], 0), torch.cat([sd[f"{a}.linear_{n}.bias"] for n in "qkv"], 0),
                                      name=a + ".linear_{q,k,v}.weight")
            lay["E"] = self._dev_f32(sd[a + ".distance_embedding.weight"])
            lay["dw_ln"] = self._ln_pair(sd, c + ".depthwise_layer_norm")
            self.layers.append(lay)
        self._arenas = SlotArenas(self._build_arena)

    def frames(self, num_samples: int) -> int:
        return self.geo.frames_for(num_samples)

    # ------------------------------------------------------------------ buffers
    def _build_arena(self, cap: Dict[str, int]) -> dict:
        """buffer set of one slot (pointers fixed between batches: the command list is recorded once per arena); ``cap``: frames M,
        utterances B, mel frames F"""
        M, B, Fr, geo, dev = cap["M"], cap["B"], cap["F"], self.geo, self.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ar = {}
        ar["mel"], ar["fb"] = f32(Fr, geo.fbank_mels), f32(M, self.fdim)
        ar["fb_act"] = self._new_act(M, self.fpad, zero=True)                 # columns past 160 stay zero
        self._conformer_buffers(ar, M)
        ar["qe"] = f32(M * geo.heads, self.qe_ld)
        ar["tab"] = TableBlob(B, 3, dev)                                     # sample_offs | mel_offs (int32) | frame_offs (int32)
        if self.fp16_planes:
            ar["range_flag"] = torch.zeros(1, dtype=torch.int32, device=dev)
        return ar

    def _plan(self, lengths: Sequence[int], slot: int = 0) -> dict:
        from .frontend import W2VBERT_MIN_SAMPLES, w2vbert_mel_frames
        lengths = tuple(int(n) for n in lengths)
        B, stride = len(lengths), self.geo.fbank_stride
        Fr = [w2vbert_mel_frames(n) for n in lengths]
        if B == 0 or min(Fr) < max(2, stride):
            raise ValueError(f"utterance shorter than {W2VBERT_MIN_SAMPLES} samples: it has no stacked fbank row")
        T = [f // stride for f in Fr]
        offs = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
        moffs = np.concatenate([[0], np.cumsum(Fr)]).astype(np.int64)
        M, Tmax, Fmax = int(offs[-1]), max(T), max(Fr)
        ar = self._arenas.fit(slot, M=M, B=B, F=int(moffs[-1]))
        if ar["plan"] is not None and ar["plan"]["lengths"] == lengths:
            return ar["plan"]
        tab = ar["tab"].begin()
        so, mo, fo = tab.put64(np.concatenate([[0], np.cumsum(lengths)])), tab.put32(moffs), tab.put32(offs)
        tab.send()
        pl = dict(ar)
        pl.update(lengths=lengths, B=Sz(B, "B"), M=Sz(M, "M"), MH=Sz(M * self.geo.heads, "MH"), Tmax=Sz(Tmax, "Tmax"), Fmax=Sz(Fmax, "Fmax"),
                  sizes=dict(B=B, M=M, MH=M * self.geo.heads, Tmax=Tmax, Fmax=Fmax), sample_offs=so, frame_offs=fo,
                  mel_offs=mo, frame_offs_host=[int(v) for v in offs], states=ar["states"][:, :M])
        ar["plan"] = pl
        return pl

    # ------------------------------------------------------------------ launches
    def _fbank(self, pl, packed_wave: torch.Tensor) -> None:
        geo = self.geo
        a = self._cmd("fbank")
        a.wav, a.sample_offs, a.mel_offs, a.frame_offs = packed_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["mel_offs"].data_ptr(), pl["frame_offs"].data_ptr()
        a.dft, a.melw, a.mel_range, a.work = self.dft.data_ptr(), self.melw.data_ptr(), self.mel_range.data_ptr(), pl["mel"].data_ptr()
        a.out, a.ldo = pl["fb"].data_ptr(), self.fdim
        a.B, a.max_mel_frames, a.n_mels, a.stride = pl["B"], pl["Fmax"], geo.fbank_mels, geo.fbank_stride
        self._issue(_lib.OP_FBANK, a, "ser_fbank", input="wav", B=pl["B"], max_mel_frames=pl["Fmax"])

    def _relkey_attention(self, pl, lay, scale: float) -> None:
        """LN rows -> packed projection -> the relative-key table per (row, head) -> ser_attention_rk_v"""
        geo = self.geo
        M, D, qkv = pl["M"], geo.hidden, pl["qkv"]
        self._layernorm(pl["r1"], D, lay["attn_ln"], M, D, out_act=pl["xa"])
        self._gemm(pl["xa"], lay["qkv"], M, out_act=qkv, col_scale=scale, col_scale_end=D)
        t = self._cmd("relkey_table")
        t.qkv, t.ld, t.plane_stride, t.E, t.qe, t.ld_qe = qkv.ptr, qkv.cols, qkv.plane_stride, lay["E"].data_ptr(), pl["qe"].data_ptr(), self.qe_ld
        t.q_col, t.rows, t.H, t.dh, t.P, t.mode = 0, M, geo.heads, geo.head_dim, geo.distance_positions, self.mode
        self._issue(_lib.OP_RELKEY_TABLE, t, "ser_relkey_table", rows=M)
        r = self._biased_attention_cmd(pl, "attention_rk")
        r.qe, r.ld_qe, r.left_max, r.right_max = pl["qe"].data_ptr(), self.qe_ld, geo.left_max_positions, geo.right_max_positions
        self._issue(_lib.OP_ATTENTION_RK, r, "ser_attention_rk")

    def _launches(self, pl, packed_wave: torch.Tensor, last_state: Optional[int] = None) -> None:
        M = pl["M"]
        self._fbank(pl, packed_wave)
        self._layernorm(pl["fb"], self.fdim, self.proj_ln, M, self.fdim, out_act=pl["fb_act"])
        self._gemm(pl["fb_act"], self.proj, M, out_f32=pl["states"][0], ldo_f32=self.geo.hidden)
        if not self._state_done(0, last_state):
            self._conformer_layers(pl, self._relkey_attention, last_state)

    @_on_stream
    def forward(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0,
                last_state: Optional[int] = None) -> HiddenStates:
        """packed 16 kHz samples [sum(lengths)] fp32 on the device -> L + 1 hidden states"""
        pl = self._plan(lengths, slot)
        return self._launch_or_replay(self._arenas[slot], pl, packed_wave, self._check_last_state(last_state))

    @_on_stream
    def fbank(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0) -> torch.Tensor:
        """the stacked, normalised fbank rows [M, 160] alone (ser_fbank_v)"""
        pl = self._plan(lengths, slot)
        self._fbank(pl, packed_wave)
        return pl["fb"][: int(pl["M"])]


class ConformerSpeechEncoder(_ConformerLayers, SpeechEncoder):
    """The wav2vec2-conformer encoders (HF Wav2Vec2ConformerModel; not in the reference, whose heads take any [T, D] stream) on libserhip:
    ``SpeechEncoder``'s layer-norm conv stem and feature projection -- hidden_states[0], there is no positional convolution -- and
    ``_ConformerLayers``' layer
        x += FFN1(LN x) / 2;  x += Attn(LN x);  x += Conv(x);  x += FFN2(LN x) / 2;  x = LN x
    with ser_conformer_conv_bn_v (centred window, BatchNorm in eval folded to a per-channel affine at load) in the convolution module, the
    layers' own LayerNorm eps of 1e-5 (nn.LayerNorm's default, whatever the config says) and one of two position schemes
    (``geo.position_type``, include/ser_hip.h a35):
      "rotary"    ser_rope_rows_v rotates the layer-normed rows; q | k are projected from the rotated planes and v from the plain ones into
                  one packed buffer, then ser_attention_v;
      "relative"  one packed projection whose q carries pos_bias_u, P = linear_pos(pe) by ser_gemm in fixed 256-row chunks anchored at
                  distance 0 (a row of P has the same bits whatever the table's length), ser_relpos_bias_v, ser_attention_rb_v.
    hidden_states[i < L] is layer i's input, hidden_states[L] = encoder.layer_norm of the last layer's output.  Every utterance alone."""

    P_CHUNK = 256            # rows per launch of the P GEMM, and the granule of the distance table's half-length
    LN_EPS = 1e-5            # the layer's own norms: nn.LayerNorm's default, whatever the config says

    def __init__(self, geo: EncoderGeometry, state_dict, device="cuda:0", mode: str = "f16x", normalize: bool = True):
        from .weights import fold_batch_norm, fold_pos_bias_u, rotary_inv_freq
        _WaveIO.__init__(self, geo, device, mode, post_ln=True)       # the conformer modes are the post-LayerNorm encoders': f16x, fp32x, bf16
        if geo.family != FAMILY_W2V_CONFORMER:
            raise ValueError(f"ConformerSpeechEncoder runs the {FAMILY_W2V_CONFORMER} family")
        self.normalize = bool(normalize)
        sd = state_dict
        H, dh = geo.heads, geo.head_dim
        if geo.position_type not in ("rotary", "relative"):
            raise ValueError(f"position type '{geo.position_type}' is not built (rotary / relative)")
        if geo.feat_extract_norm != "layer":
            raise NotImplementedError("the conformer encoders are built behind the layer-norm conv stem")
        self._check_conformer_geometry("conformer")
        self.relative = geo.position_type == "relative"
        self._init_stem(sd)
        self.enc_ln = self._ln_pair(sd, "encoder.layer_norm")
        scale = self._q_scale()                                        # what the projection's col_scale gives q
        if not self.relative:
            inv = sd.get("encoder.embed_positions.inv_freq")           # a checkpoint stores HF's buffer; synthetic weights do not
            self.inv_freq = (inv.detach().float().cpu() if inv is not None else rotary_inv_freq(dh, geo.rotary_base))
            if tuple(self.inv_freq.shape) != (dh // 2,):
                raise ValueError(f"encoder.embed_positions.inv_freq: shape {tuple(self.inv_freq.shape)}, expected ({dh // 2},)")
        self._pe: Dict[int, Act] = {}                                  # half-length of the distance table -> operand planes of its pe rows
        self.layers = []
        for i in range(geo.num_layers):
            a, bn = f"encoder.layers.{i}.self_attn", f"encoder.layers.{i}.conv_module.batch_norm"
            lay = self._conformer_layer_weights(sd, i)
            w = {n: sd[f"{a}.linear_{n}.weight"] for n in "qkv"}
            b = {n: sd[f"{a}.linear_{n}.bias"] for n in "qkv"}
            if self.relative:
                u, v = sd[a + ".pos_bias_u"], sd[a + ".pos_bias_v"]
                if tuple(u.shape) != (H, dh) or tuple(v.shape) != (H, dh):
                    raise ValueError(f"{a}.pos_bias_u / pos_bias_v: shapes {tuple(u.shape)} / {tuple(v.shape)}, expected ({H}, {dh})")
                lay["qkv"] = self._linear(torch.cat([w[n] for n in "qkv"], 0), torch.cat([fold_pos_bias_u(b["q"], u), b["k"].float(), b["v"].float()], 0),
                                          name=a + ".linear_{q,k,v}.weight")
                lay["pos"] = self._linear(sd[a + ".linear_pos.weight"], None, name=a + ".linear_pos.weight")
                lay["off"] = self._dev_f32(((v.detach().double() - u.detach().double()) * scale).reshape(-1).float())
            else:
                lay["qk"] = self._linear(torch.cat([w["q"], w["k"]], 0), torch.cat([b["q"], b["k"]], 0), name=a + ".linear_{q,k}.weight")
                lay["v"] = self._linear(w["v"], b["v"], name=a + ".linear_v.weight")
            lay["bn"] = tuple(self._dev_f32(t) for t in fold_batch_norm(sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                                                                        sd[bn + ".running_var"], 1e-5))      # nn.BatchNorm1d's own eps
            self.layers.append(lay)
        self._arenas = SlotArenas(self._build_arena)

    def frames(self, num_samples: int) -> int:
        return self.geo.frames_for(num_samples)

    # ------------------------------------------------------------------ buffers
    def _pe_rows(self, Tp: int) -> Act:
        """operand planes of pe(r), r = -Tp .. Tp - 1 (row Tp + r): uploaded once per table length"""
        act = self._pe.get(Tp)
        if act is None:
            from .weights import relpos_pe
            pe = relpos_pe(Tp + 1, self.geo.hidden)[: 2 * Tp].contiguous().to(self.device)
            act = self._new_act(2 * Tp, self.geo.hidden)
            check(lib.ser_split_bf16(pe.data_ptr(), act.ptr, pe.numel(), self.mode, act.plane_stride, _stream()), "ser_split_bf16")
            torch.cuda.current_stream().synchronize()
            self._pe[Tp] = act
        return act

    def _build_arena(self, cap: Dict[str, int]) -> dict:
        """buffer set of one slot; ``cap``: the stem's rows, frames M, utterances B, longest utterance Tmax (sizes the position tables)"""
        from .weights import rotary_tables
        M, B, geo, dev = cap["M"], cap["B"], self.geo, self.device
        D, H = geo.hidden, geo.heads
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ar = {}
        self._stem_arena(ar, cap)
        self._conformer_buffers(ar, M)
        ar["last"] = f32(M, D)
        if self.relative:
            Tp = -(-cap["Tmax"] // self.P_CHUNK) * self.P_CHUNK
            ar["P_T"], ar["pe"], ar["P"] = Tp, self._pe_rows(Tp), f32(2 * Tp, D)
            ar["ld_pb"] = -(-cap["Tmax"] // 64) * 64
            ar["pb"] = f32(M * H, ar["ld_pb"])
        else:
            cos, sin = rotary_tables(cap["Tmax"], self.inv_freq)
            ar["table_T"], ar["cos"], ar["sin"] = cap["Tmax"], cos.to(dev), sin.to(dev)
            ar["ln"], ar["xr"] = f32(M, D), self._new_act(M, D)
        ar["tab"] = TableBlob(B, 2 * len(geo.conv_dim), dev)                 # sample_offs | offs[0..nl) (int32) | conv bases [1..nl)
        if self.fp16_planes:
            ar["range_flag"] = torch.zeros(1, dtype=torch.int32, device=dev)
        return ar

    def _plan(self, lengths: Sequence[int], slot: int = 0) -> dict:
        lengths = tuple(int(n) for n in lengths)
        B, H = len(lengths), self.geo.heads
        offs = self._stem_offsets(lengths)
        M, Tmax = int(offs[-1][-1]), int(np.diff(offs[-1]).max())
        ar = self._arenas.fit(slot, rows0=int(offs[0][-1]), rows1=int(offs[1][-1]) if len(offs) > 1 else 1, M=M, B=B, Tmax=Tmax)
        if ar["plan"] is not None and ar["plan"]["lengths"] == lengths:
            return ar["plan"]
        tab = ar["tab"].begin()
        pl = dict(ar)
        offs_dev, base_conv = self._stem_tables(pl, tab, lengths, offs)
        tab.send()
        pl["sizes"].update(M=M, B=B, Tmax=Tmax)
        pl.update(B=Sz(B, "B"), lengths=lengths, M=Sz(M, "M"), Tmax=Sz(Tmax, "Tmax"), states=ar["states"][:, :M])
        self._stem_index(pl, ar, offs_dev, base_conv, _stream())
        ar["plan"] = pl
        return pl

    # ------------------------------------------------------------------ launches
    def _rotary_attention(self, pl, lay, scale: float) -> None:
        """LN rows (fp32 ``ln`` + plain planes ``xa``) -> rotated planes -> q | k from them, v from the plain ones -> ser_attention_v"""
        geo = self.geo
        M, D, out = pl["M"], geo.hidden, pl["xr"]
        self._layernorm(pl["r1"], D, lay["attn_ln"], M, D, out_f32=pl["ln"], out_act=pl["xa"], eps=self.LN_EPS)
        a = self._cmd("rope_rows")
        a.x, a.ldx, a.cos_t, a.sin_t, a.frame_offs = pl["ln"].data_ptr(), D, pl["cos"].data_ptr(), pl["sin"].data_ptr(), pl["frame_offs"].data_ptr()
        a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = out.ptr, out.cols, out.plane_stride, self._flag
        a.B, a.rows, a.D, a.dh, a.table_T, a.max_frames, a.mode = pl["B"], M, D, geo.head_dim, pl["table_T"], pl["Tmax"], self.mode
        self._issue(_lib.OP_ROPE_ROWS, a, "ser_rope_rows", B=pl["B"], rows=M, max_frames=pl["Tmax"])
        self._gemm(pl["xr"], lay["qk"], M, out_act=pl["qkv"], col_scale=scale, col_scale_end=D)
        self._gemm(pl["xa"], lay["v"], M, out_act=pl["qkv"], out_col=2 * D)
        self._attention(pl["qkv"], pl["frame_offs"], pl["B"], pl["Tmax"], pl["ctx"])

    def _relative_attention(self, pl, lay, scale: float) -> None:
        """LN rows -> packed projection (q carries pos_bias_u) -> P = linear_pos(pe) -> the positional term per (row, head, key) ->
        ser_attention_rb_v"""
        geo = self.geo
        M, D, H, Tp = pl["M"], geo.hidden, geo.heads, pl["P_T"]
        qkv, pe = pl["qkv"], pl["pe"]
        self._layernorm(pl["r1"], D, lay["attn_ln"], M, D, out_act=pl["xa"], eps=self.LN_EPS)
        self._gemm(pl["xa"], lay["qkv"], M, out_act=qkv, col_scale=scale, col_scale_end=D)
        for r0 in range(0, 2 * Tp, self.P_CHUNK):
            self._gemm(pe, lay["pos"], self.P_CHUNK, a_ptr_offset=2 * r0 * pe.cols, out_f32=pl["P"][r0: r0 + self.P_CHUNK], ldo_f32=D)
        t = self._cmd("relpos_bias")
        t.qkv, t.ld, t.plane_stride, t.P, t.ldp, t.off = qkv.ptr, qkv.cols, qkv.plane_stride, pl["P"].data_ptr(), D, lay["off"].data_ptr()
        t.frame_offs, t.pb, t.ld_pb = pl["frame_offs"].data_ptr(), pl["pb"].data_ptr(), pl["ld_pb"]
        t.q_col, t.B, t.H, t.dh, t.P_T, t.max_frames, t.rows, t.mode = 0, pl["B"], H, geo.head_dim, Tp, pl["Tmax"], M, self.mode
        self._issue(_lib.OP_RELPOS_BIAS, t, "ser_relpos_bias", B=pl["B"], max_frames=pl["Tmax"], rows=M)
        r = self._biased_attention_cmd(pl, "attention_rb")
        r.pb, r.ld_pb = pl["pb"].data_ptr(), pl["ld_pb"]
        self._issue(_lib.OP_ATTENTION_RB, r, "ser_attention_rb")

    def _launches(self, pl, packed_wave: torch.Tensor, last_state: Optional[int] = None) -> None:
        self._conv_stack(pl, packed_wave)
        self._gemm(pl["feat_act"], self.proj, pl["M"], out_f32=pl["states"][0], ldo_f32=self.geo.hidden, stem=True)
        if not self._state_done(0, last_state):
            self._conformer_layers(pl, self._relative_attention if self.relative else self._rotary_attention, last_state,
                                   eps=self.LN_EPS, enc_ln=self.enc_ln)

    @_on_stream
    def forward(self, packed_wave: torch.Tensor, lengths: Sequence[int], slot: int = 0,
                last_state: Optional[int] = None) -> HiddenStates:
        """packed raw samples [sum(lengths)] fp32 on the device -> L + 1 hidden states"""
        pl = self._plan(lengths, slot)
        return self._launch_or_replay(self._arenas[slot], pl, packed_wave, self._check_last_state(last_state))


def build_encoder(geo: EncoderGeometry, state_dict, device="cuda:0", mode="bf16", normalize: bool = True):
    """``normalize``: the speech families' input normalisation (``do_normalize`` of the checkpoint's feature extractor)."""
    if geo.family == "deberta":
        return DebertaEncoder(geo, state_dict, device, mode)
    if geo.family == FAMILY_ROBERTA:
        return TextEncoder(geo, state_dict, device, mode)
    if geo.family == FAMILY_WHISPER:
        return WhisperEncoder(geo, state_dict, device, mode)
    if geo.family == FAMILY_W2V_BERT:
        return W2vBertEncoder(geo, state_dict, device, mode)
    if geo.family == FAMILY_W2V_CONFORMER:
        return ConformerSpeechEncoder(geo, state_dict, device, mode, normalize=normalize)
    return SpeechEncoder(geo, state_dict, device, mode, normalize=normalize)
