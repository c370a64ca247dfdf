"""numpy restatement of the streaming joint Viterbi (TEST INFRASTRUCTURE): the e2vq_hmm_segment_stream_* session and `hmm
segment --continuous`, DESIGN.md 4.8.9.

What is stated here, as plain code: the block schedule (blocks of exactly B frames, the remainder buffered), the carry (a
block starts from the d the previous one left; the frame-0 rule at the absolute frame 0 only), the finality rule (the paths of
all live states followed back in lockstep to the latest frame where they are in one state, the join with the previous commit),
the status rules and the cap on the pending frames.  The recursion of one frame is hmm_segment_restatement's contract, one
class at a time; the tests hold this file against `segment_logs` / `transcribe` of that module on the concatenation.
"""
import numpy as np

from .hmm_segment_restatement import ENTER, NINF


class RingFull(Exception):
    """the next block does not fit the pending frames; .taken: symbols of the feed that were processed"""

    def __init__(self, pending, taken):
        super().__init__(f"{pending} frames are pending")
        self.pending, self.taken = pending, taken


class BadSymbol(Exception):
    """a symbol >= M; .frame: its absolute frame"""

    def __init__(self, frame):
        super().__init__(f"symbol outside the alphabet at frame {frame}")
        self.frame = frame


class Stream:
    """One session.  lms = [(lpi, lA, lB)]; B: frames of a block; cap: the pending frames the budget holds (None: no bound).
    feed / flush / close return the frames that became final with the call as a dict first, cls, state, entered, gbest.
    The whole history is kept (this is a restatement, not the ring): `final_after(p)` answers for any p processed so far."""

    def __init__(self, lms, ln_switch, B=4096, cap=None):
        assert B >= 1 and (cap is None or cap >= 2 * B)
        self.lms, self.ls, self.B, self.cap = lms, float(ln_switch), int(B), cap
        self.M = lms[0][2].shape[1]
        Ns = [len(m[0]) for m in lms]
        self.comp0 = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
        self.owner = np.concatenate([np.full(N, k) for k, N in enumerate(Ns)])
        self.buf = []            # the buffered remainder
        self.fed = 0             # symbols given
        self.p = 0               # frames processed
        self.F = 0               # frames final
        self.dirty = False       # frames were processed since the last coalescence
        self.d = None            # d of frame p - 1, composite order
        self.psi, self.g, self.G, self.ds = [], [], [], []  # per processed frame (psi / g of frame 0: None)
        self.prev_a = None
        self.join_failures = 0
        self.peak_pending = 0
        self.status, self.log_prob, self.closed, self.bad_frame = 0, None, False, None
        self.cls, self.state, self.entered, self.gbest = [], [], [], []  # of the final frames

    # ---- the recursion of one frame (hmm_segment_restatement's contract, a class at a time) -------------------------------
    def _step(self, o):
        if self.p == 0:
            nd = np.concatenate([lpi + lB[:, o] for lpi, _lA, lB in self.lms])
            psi, g, G = None, None, 0.0
        else:
            d = self.d
            g = int(np.argmax(d))  # (the first maximum: the lowest composite index)
            G = float(d[g])
            base = G + self.ls
            nd, psi = np.empty_like(d), np.empty(len(d), dtype=np.int64)
            for k, (lpi, lA, lB) in enumerate(self.lms):
                a, b = self.comp0[k], self.comp0[k + 1]
                v = d[a:b, None] + lA  # v[i, j] = d[i] + lA[i][j]
                arg = np.argmax(v, axis=0)
                best = v[arg, np.arange(b - a)]
                x = base + lpi
                ent = x > best
                psi[a:b] = np.where(ent, ENTER, arg)
                nd[a:b] = np.where(ent, x, best) + lB[:, o]
        self.d = nd
        self.psi.append(psi)
        self.g.append(g)
        self.G.append(G)
        self.ds.append(nd)
        self.p += 1

    def _back(self, t, q):
        """the composite state at frame t - 1 of the path that is in q at frame t >= 1"""
        a = self.psi[t][q]
        return self.g[t] if a == ENTER else int(self.comp0[self.owner[q]] + a)

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
        stream that has not died: a dead one decides nothing more, and what it decided before depends on when it was asked)"""
        if p == 0:
            return 0
        r = self._coalesce(p - 1, 0)
        return 0 if r is None else r[0] + 1

    def _decide(self, f, a):
        """the frames F .. f become final: the backtrack from (f, a); the state it reaches at F - 1 joins the previous commit"""
        F = self.F
        n = f - F + 1
        cls, state, entered = [0] * n, [0] * n, [0] * n
        q = a
        for t in range(f, F - 1, -1):
            k = int(self.owner[q])
            cls[t - F], state[t - F] = k, q - int(self.comp0[k])
            if t == 0:
                entered[0] = 1
                break
            entered[t - F] = 1 if self.psi[t][q] == ENTER else 0
            q = self._back(t, q)
        if F > 0 and self.status == 0 and self.prev_a is not None and q != self.prev_a:
            self.join_failures += 1
        self.prev_a = a
        out = dict(first=F, cls=cls, state=state, entered=entered, gbest=self.G[F:f + 1])
        self.cls += cls
        self.state += state
        self.entered += entered
        self.gbest += out["gbest"]
        self.F = f + 1
        return out

    def _commit(self):
        """one coalescence over the pending frames"""
        self.dirty = False
        if self.p > self.F:
            r = self._coalesce(self.p - 1, self.F)
            if r is not None and r[0] >= self.F:
                return self._decide(*r)
        return dict(first=self.F, cls=[], state=[], entered=[], gbest=[])

    @staticmethod
    def _join(outs):
        outs = [o for o in outs if o["cls"]] or outs[-1:]
        return dict(first=outs[0]["first"], **{k: sum((o[k] for o in outs), []) for k in ("cls", "state", "entered", "gbest")})

    # ---- the schedule ------------------------------------------------------------------------------------------------------
    def _block(self, syms):
        for i, o in enumerate(syms):
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
        """-> the rest of the frames; self.log_prob and self.status are set"""
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
            out = dict(first=self.F, cls=[0xFFFF] * n, state=[0xFFFF] * n, entered=[0] * n, gbest=[NINF] * n)
            self.cls += out["cls"]
            self.state += out["state"]
            self.entered += out["entered"]
            self.gbest += out["gbest"]
            self.F, self.log_prob = self.fed, NINF
            return out
        if self.p == 0:
            self.log_prob = 0.0
            return dict(first=0, cls=[], state=[], entered=[], gbest=[])
        q = int(np.argmax(self.d))  # (the lowest composite index reaching max d)
        self.log_prob = float(self.d[q])
        self.status = 1 if self.log_prob == NINF else 0
        if self.p > self.F:
            return self._decide(self.p - 1, q)
        return dict(first=self.F, cls=[], state=[], entered=[], gbest=[])


def decode(lms, seq, ln_switch, B, feeds, cap=None):
    """the session fed seq in pieces of the lengths `feeds` (their sum: len(seq)), then closed -> (Stream, the number of final
    frames after each feed)"""
    s = Stream(lms, ln_switch, B, cap)
    at, finals = 0, []
    for n in feeds:
        s.feed(seq[at:at + n])
        at += n
        finals.append(s.F)
    assert at == len(seq)
    s.close()
    return s, finals
