"""numpy restatement of the streaming joint Viterbi under class-to-class prices (TEST INFRASTRUCTURE): a session opened by
e2vq_hmm_segment_trans_stream_open and `hmm segment --class-transitions --grammar-continuous`, DESIGN.md 4.8.15.

What is stated here, as plain code: the block schedule, the carry, the status rules and the cap of
hmm_segment_stream_restatement (4.8.9), with the recursion of one frame and the back step of hmm_segment_trans_restatement
(4.8.8): state (k, j) at frame t goes to (k, psi), or on ENTER to (src_t[k], x_t[src_t[k]]).  The tests hold this file against
`segment_trans_logs` / `transcribe` of that module on the concatenation.
"""
import numpy as np

from .hmm_segment_stream_restatement import BadSymbol, RingFull  # noqa: F401 (the callers catch them)
from .hmm_segment_trans_restatement import ENTER, NINF

KEYS = ("cls", "state", "entered", "exit_score")


def _none(first):
    return dict(first=first, cls=[], state=[], entered=[], exit_score=[])


class Stream:
    """One session.  lms = [(lpi, lA, lB)]; lt: the K x K prices; B: frames of a block; cap: the pending frames the budget
    holds (None: no bound).  feed / flush / close return the frames that became final with the call as a dict first, cls,
    state, entered, exit_score.  The whole history is kept (this is a restatement, not the ring): `final_after(p)` answers
    for any p processed so far."""

    def __init__(self, lms, lt, B=4096, cap=None):
        assert B >= 1 and (cap is None or cap >= 2 * B)
        self.lms, self.lt, self.B, self.cap = lms, np.asarray(lt, dtype=np.float64), int(B), cap
        self.K = len(lms)
        self.M = lms[0][2].shape[1]
        Ns = [len(m[0]) for m in lms]
        self.comp0 = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
        self.owner = np.concatenate([np.full(N, k) for k, N in enumerate(Ns)])
        self.lpi = np.concatenate([m[0] for m in lms])
        self.buf = []            # the buffered remainder
        self.fed = 0             # symbols given
        self.p = 0               # frames processed
        self.F = 0               # frames final
        self.dirty = False       # frames were processed since the last coalescence
        self.d = None            # d of frame p - 1, composite order
        self.psi, self.src, self.xs, self.Es, self.ds = [], [], [], [], []  # per processed frame (frame 0: None but ds)
        self.prev_a = None
        self.join_failures = 0
        self.peak_pending = 0
        self.status, self.log_prob, self.closed, self.bad_frame = 0, None, False, None
        self.cls, self.state, self.entered, self.exit_score = [], [], [], []  # of the final frames

    # ---- the recursion of one frame (hmm_segment_trans_restatement's contract) -------------------------------------------
    def _step(self, o):
        K = self.K
        if self.p == 0:
            nd = np.concatenate([lpi + lB[:, o] for lpi, _lA, lB in self.lms])
            psi = src = xs = Es = None
        else:
            d = self.d
            parts = [d[self.comp0[k]:self.comp0[k + 1]] for k in range(K)]
            xs = np.array([int(np.argmax(p)) for p in parts])  # (the first maximum: the lowest state)
            Es = np.array([p[i] for p, i in zip(parts, xs)])
            with np.errstate(invalid="ignore"):
                v = Es[:, None] + self.lt  # v[f, k] = E[f] + lt[f][k]
                src = np.argmax(v, axis=0)  # (the lowest source class wins ties)
                base = v[src, np.arange(K)]
                enter = base[self.owner] + self.lpi
                nd, psi = np.empty_like(d), np.empty(len(d), dtype=np.int64)
                for k, (_lpi, lA, lB) in enumerate(self.lms):
                    a, b = self.comp0[k], self.comp0[k + 1]
                    w = parts[k][:, None] + lA  # w[i, j] = d[k][i] + lA_k[i][j]
                    arg = np.argmax(w, axis=0)
                    best = w[arg, np.arange(b - a)]
                    ent = enter[a:b] > best
                    psi[a:b] = np.where(ent, ENTER, arg)
                    nd[a:b] = np.where(ent, enter[a:b], best) + lB[:, o]
        self.d = nd
        self.psi.append(psi)
        self.src.append(src)
        self.xs.append(xs)
        self.Es.append(Es)
        self.ds.append(nd)
        self.p += 1

    def _back(self, t, q):
        """the composite state at frame t - 1 of the path that is in q at frame t >= 1"""
        a = self.psi[t][q]
        k = int(self.owner[q])
        if a == ENTER:
            f = int(self.src[t][k])
            return int(self.comp0[f] + self.xs[t][f])
        return int(self.comp0[k] + a)

    # ---- finality -----------------------------------------------------------------------------------------------------------
    def _coalesce(self, e, lowest):
        """(f*, a): the latest frame in [lowest, e] at which the paths from all live states of frame e are in one state, or None"""
        qs = set(int(c) for c in np.flatnonzero(self.ds[e] > NINF))
        if not qs:
            return None
        t = e
        while True:
            if len(qs) == 1:
                return t, next(iter(qs))
            if t <= lowest:  # (the walk never leaves the pending frames)
                return None
            qs = set(self._back(t, q) for q in qs)
            t -= 1

    def final_after(self, p):
        """the number of final frames after p <= self.p processed frames: a function of the first p symbols alone (for a
        stream that has not died)"""
        if p == 0:
            return 0
        r = self._coalesce(p - 1, 0)
        return 0 if r is None else r[0] + 1

    def _decide(self, f, a):
        """the frames F .. f become final: the backtrack from (f, a); the state it reaches at F - 1 joins the previous commit.
        exit_score[t] = E_t of the class of frame t - 1, which for t = F is the class of the state reached there"""
        F = self.F
        n = f - F + 1
        cls, state, entered, ex = [0] * n, [0] * n, [0] * n, [0.0] * n
        q = a
        for t in range(f, F - 1, -1):
            k = int(self.owner[q])
            cls[t - F], state[t - F] = k, q - int(self.comp0[k])
            if t == 0:
                entered[0], ex[0] = 1, 0.0
                break
            entered[t - F] = 1 if self.psi[t][q] == ENTER else 0
            q = self._back(t, q)
            ex[t - F] = float(self.Es[t][self.owner[q]])
        if F > 0 and self.status == 0 and self.prev_a is not None and q != self.prev_a:
            self.join_failures += 1
        self.prev_a = a
        out = dict(first=F, cls=cls, state=state, entered=entered, exit_score=ex)
        for k in KEYS:
            getattr(self, k).extend(out[k])
        self.F = f + 1
        return out

    def _commit(self):
        """one coalescence over the pending frames"""
        self.dirty = False
        if self.p > self.F:
            r = self._coalesce(self.p - 1, self.F)
            if r is not None and r[0] >= self.F:
                return self._decide(*r)
        return _none(self.F)

    @staticmethod
    def _join(outs):
        outs = [o for o in outs if o["cls"]] or outs[-1:]
        return dict(first=outs[0]["first"], **{k: sum((o[k] for o in outs), []) for k in KEYS})

    # ---- the schedule (hmm_segment_stream_restatement's) -----------------------------------------------------------------
    def _block(self, syms):
        for o in syms:
            if o >= self.M:
                self.status, self.bad_frame = 2, self.p
                raise BadSymbol(self.p)
            self._step(int(o))
        self.dirty = True
        self.peak_pending = max(self.peak_pending, self.p - self.F)

    def _make_room(self, n, outs, taken):
        if self.cap is None or self.p - self.F + n <= self.cap:
            return
        if self.dirty:
            outs.append(self._commit())
        if self.p - self.F + n > self.cap:
            raise RingFull(self.p - self.F, taken)

    def feed(self, seq):
        assert not self.closed and self.status != 2
        seq = [int(x) for x in seq]
        outs, o = [], 0
        try:
            while len(self.buf) + (len(seq) - o) >= self.B:
                self._make_room(self.B, outs, o)
                take = self.B - len(self.buf)
                blk = self.buf + seq[o:o + take]
                self._block(blk)
                o += take
                self.buf = []
        except BadSymbol:
            self.fed += len(seq)  # (all of the failing feed counts as fed)
            self.buf = []
            raise
        except RingFull:
            self.fed += o  # (the rest of the feed is dropped)
            self.pending_out = self._join(outs) if outs else None
            raise
        self.buf += seq[o:]
        self.fed += len(seq)
        outs.append(self._commit())
        return self._join(outs)

    def flush(self):
        assert not self.closed and self.status != 2
        outs = []
        if self.buf:
            self._make_room(len(self.buf), outs, 0)
            blk, self.buf = self.buf, []
            self._block(blk)
        outs.append(self._commit())
        return self._join(outs)

    def close(self):
        """-> the rest of the frames; self.log_prob and self.status are set.  Status 2: every frame that was not final is
        filled with 0xFFFF, 0xFFFF, 0 and exit_score -inf -- 0.0 at the absolute frame 0, as the closed decode fills it"""
        assert not self.closed
        self.closed = True
        if self.status != 2 and self.buf:
            blk, self.buf = self.buf, []
            try:
                self._block(blk)  # (beyond the cap: the ring keeps B - 1 rows for this)
            except BadSymbol:
                pass
        if self.status == 2:
            n = self.fed - self.F
            out = dict(first=self.F, cls=[0xFFFF] * n, state=[0xFFFF] * n, entered=[0] * n, exit_score=[NINF] * n)
            if self.F == 0 and n > 0:
                out["exit_score"][0] = 0.0
            for k in KEYS:
                getattr(self, k).extend(out[k])
            self.F, self.log_prob = self.fed, NINF
            return out
        if self.p == 0:
            self.log_prob = 0.0
            return _none(0)
        q = int(np.argmax(self.d))  # (the lowest composite index reaching max d)
        self.log_prob = float(self.d[q])
        self.status = 1 if self.log_prob == NINF else 0
        if self.p > self.F:
            return self._decide(self.p - 1, q)
        return _none(self.F)


def decode(lms, seq, lt, B, feeds, cap=None):
    """the session fed seq in pieces of the lengths `feeds` (their sum: len(seq)), then closed -> (Stream, the number of final
    frames after each feed)"""
    s = Stream(lms, lt, B, cap)
    at, finals = 0, []
    for n in feeds:
        s.feed(seq[at:at + n])
        at += n
        finals.append(s.F)
    assert at == len(seq)
    s.close()
    return s, finals
