"""The beam search rule (numpy, float64): ``GenerationMixin._beam_search`` of transformers 5.15 (generation/utils.py) restated for
do_sample=False, early_stopping=False, num_return_sequences=1, one eos token and any length_penalty, one utterance at a time.

One step, with ``cur`` tokens in every row (HF's cur_len) and the fp32 logits z [K, V] of the K running rows:

    logp   = z - logsumexp(z)                    over the RAW logits: suppressed tokens count in the normaliser
    masked : the suppress sets (steady; begin-suppress too at the first generated position) are taken out AFTER the log-softmax
    acc    = logp + run[k]                       run starts as [0, dead, dead, ...]: at the first step only beam 0 is alive
    top 2K of the K V values; parent = index // V, token = index % V.  Fewer than 2K finite candidates is an ERROR, not a tie-break
    hit    = token == eos or cur + 1 == max_length
    running beams of the next step: the best K candidates that did not hit
    finished set: only candidates of rank < K that hit, acc / (cur + 1 - prompt_len) ** length_penalty, merged with the previous set, the best
             K kept; nothing enters once the early-stop flag has dropped
    flag  &= run'[0] / (cur + 1 - prompt_len) ** length_penalty > worst finished        (only once K have finished: HF compares with -1e9)
    done   = flag dropped, or every candidate hit

Masks, not -1e9.  HF marks "dead beam", "hit" and "not finished yet" by ADDING -1e9 to float scores and lets topk sort them out.  Here
they are masks: a dead beam or a suppressed token is no candidate, a hit candidate is no running beam, an empty finished slot is absent.
The two agree whenever every real accumulated score is far above -1e9 -- a sum of at most max_length log-probabilities of fp32 logits,
each above -1e3 in practice -- and at least K candidates of a step do not hit, or all hit (max_length): then every -1e9 entry sorts
behind every real one, exactly as an absent one does.  Where fewer than 2K real candidates exist HF would rank -1e9 entries among the
winners; that is the error above.  test_whisper_beam_host.py checks the agreement against HF itself.

Ties: the lower flat index parent * V + token wins; between finished scores the older entry wins (HF's CPU topk order on ties is not
pinned).  Arithmetic: float64 throughout, on fp32 logits.  A NaN logit counts as a winning +inf and fails the step (error bit 0), as in
ser_dec_select_v; after an error only the error word is specified.

``gaps``: per step the smallest gap of a comparison that decided it: the cut at rank 2K, the cut behind the K-th candidate that did
not hit, rank K - 1 against K when either hit, each finished-merge comparison against the worst kept score, both sides of the flag's
comparison.  +inf where none applied.
"""
import numpy as np

ERR_NONFINITE, ERR_POSITION, ERR_CANDIDATES = 1, 4, 8


def log_softmax64(z):
    """float64 log-softmax of fp32 logits [.., V]"""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = z.max(-1, keepdims=True)
        return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


class Beam:
    """The state of one utterance.  ``steps``: per step dict(cur, cand [(parent, token)] * 2K, cand_scores, run [(parent, token)] * K,
    run_scores, gap, finished and flag as they stood after the step); None for a step the utterance was frozen at.  ``finished``:
    [(score, (step index, rank))] best first."""

    def __init__(self, K, V, eos, pad, prompt_len, max_length, length_penalty=1.0):
        self.K, self.V, self.eos, self.pad, self.P, self.max_length, self.lp = K, V, eos, pad, prompt_len, max_length, float(length_penalty)
        self.run = np.full(K, -np.inf)
        self.run[0] = 0.0
        self.finished = []
        self.flag, self.done, self.done_step, self.err = True, False, None, 0
        self.steps = []

    def lenpow(self, n):
        return float(np.float64(n) ** np.float64(self.lp))

    def step(self, logits, cur, banned=None):
        """``logits`` fp32 [K, V]; ``banned`` bool [V]: the tokens the masks take out at this position.  A done utterance is frozen."""
        K, V = self.K, self.V
        if self.done:
            self.steps.append(None)
            return
        z = np.asarray(logits, dtype=np.float32)[:, :V]
        with np.errstate(all="ignore"):
            acc = log_softmax64(z) + self.run[:, None]
        acc = np.where(np.isnan(acc) & np.isfinite(self.run)[:, None], np.inf, acc)
        if banned is not None:
            acc = np.where(np.asarray(banned, dtype=bool)[None, :], -np.inf, acc)
        acc = np.where(np.isnan(acc), -np.inf, acc)
        flat = acc.reshape(-1)
        order = np.lexsort((np.arange(flat.size), -flat))[: 2 * K + 1]          # the larger first, then the lower flat index
        order = [int(i) for i in order if flat[i] > -np.inf]
        if len(order) < 2 * K:
            self.err |= ERR_CANDIDATES
        if any(not np.isfinite(flat[i]) for i in order[: 2 * K]):
            self.err |= ERR_NONFINITE
        if self.err:
            self.done = True
            self.steps.append(None)
            return
        gap = np.inf
        if len(order) > 2 * K:
            gap = min(gap, flat[order[2 * K - 1]] - flat[order[2 * K]])
        top = order[: 2 * K]
        score = [float(flat[i]) for i in top]
        cand = [(i // V, i % V) for i in top]
        at_max = cur + 1 >= self.max_length
        hit = [t == self.eos or at_max for _, t in cand]
        alive = [j for j in range(2 * K) if not hit[j]]
        new_run = np.full(K, -np.inf)
        run_pt = [(r, self.pad) for r in range(K)]
        for r, j in enumerate(alive[:K]):
            new_run[r], run_pt[r] = score[j], cand[j]
        if len(alive) > K:
            gap = min(gap, score[alive[K - 1]] - score[alive[K]])
        if hit[K - 1] or hit[K]:
            gap = min(gap, score[K - 1] - score[K])
        den = self.lenpow(cur + 1 - self.P)
        if self.flag:
            for j in range(K):
                if not hit[j]:
                    continue
                s = score[j] / den
                if len(self.finished) == K:
                    gap = min(gap, abs(s - self.finished[-1][0]))
                at = len(self.finished)
                while at > 0 and s > self.finished[at - 1][0]:                  # behind every entry that is not worse: the older one wins
                    at -= 1
                self.finished.insert(at, (s, (len(self.steps), j)))
                del self.finished[K:]
        if len(self.finished) == K:
            best = new_run[0] / den
            if new_run[0] > -np.inf:
                gap = min(gap, abs(best - self.finished[-1][0]))
            if not best > self.finished[-1][0]:
                self.flag = False
        self.run = new_run
        self.steps.append(dict(cur=cur, cand=cand, cand_scores=score, run=run_pt, run_scores=new_run.copy(), gap=float(gap),
                               finished=list(self.finished), flag=self.flag))
        if not self.flag or len(alive) == 0:
            self.done, self.done_step = True, len(self.steps) - 1

    # ---------------------------------------------------------------- reading the result
    def history(self, step, rank):
        """the generated tokens of candidate ``rank`` of step ``step``, by backtracking through the running beams"""
        parent, tok = self.steps[step]["cand"][rank]
        out = [tok]
        for s in range(step - 1, -1, -1):
            parent, tok = self.steps[s]["run"][parent]
            out.append(tok)
        return out[::-1]

    def running_history(self, step, row):
        """the generated tokens running row ``row`` holds after step ``step``"""
        out = []
        for s in range(step, -1, -1):
            row, tok = self.steps[s]["run"][row]
            out.append(tok)
        return out[::-1]

    def nbest(self):
        """[(generated tokens, score)] best first"""
        return [(self.history(*h), s) for s, h in self.finished]

    def final_gap(self):
        """best against second-best finished score"""
        return self.finished[0][0] - self.finished[1][0] if len(self.finished) > 1 else np.inf


def search(step_logits, K, V, eos, pad, prompt_len, max_length, length_penalty=1.0, banned=None):
    """Run one utterance to the end.  ``step_logits(beam, cur)`` -> fp32 [K, V] for the running rows (``beam.running_history``);
    ``banned(cur)`` -> bool [V] or None."""
    beam = Beam(K, V, eos, pad, prompt_len, max_length, length_penalty)
    cur = prompt_len
    while not beam.done and cur < max_length:
        beam.step(step_logits(beam, cur), cur, None if banned is None else banned(cur))
        cur += 1
    return beam
