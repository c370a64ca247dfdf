"""restatement of the posterior stream (TEST INFRASTRUCTURE): e2vq_hmm_posterior_stream_* and `hmm segment
--continuous-posteriors`, DESIGN.md 4.8.17.

There is no arithmetic here.  The K posteriors delivered for frame t of block b are row t of the closed pass
(hmm_posterior_restatement.posteriors_one) on the prefix o[0 : w_b) of everything fed, w_b = (b + 1) B + L while the stream is
open and T at close.  What this file states is the schedule -- which blocks are ready after p symbols, which prefix each is
conditioned on -- and the status rules: the first event in frame order decides, the launch whose forward pass meets it
delivers nothing, rows delivered earlier stay, every other row of everything fed comes as +0.0 with close.
"""
import numpy as np

from . import hmm_posterior_restatement as R

NINF = float("-inf")


class BadSymbol(Exception):
    """the feed (or close) that meets a symbol >= M"""

    def __init__(self, frame):
        super().__init__(f"the symbol at frame {frame} is outside the alphabet")
        self.frame = frame


class Refused(Exception):
    """a feed after close or after status 2; a second close"""


def ready_after(p, B, L):
    """the frames of a clean stream that are ready once p symbols were fed: the blocks with (b + 1) B + L <= p"""
    return B * ((p - L) // B) if p >= L else 0


class Stream:
    """models = [(pi, A, B)], one ln_switch, a block length B >= 1 and a look-ahead L >= 0.  feed(sym), close() and take()
    return (first, rows): the absolute frame of the first row that became ready with the call, and the rows (count, K).
    closed_pass: hmm_posterior_restatement.posteriors_one, or a function of its signature (the looped body's class sets
    need the one without the cap of 16 slots).  cache: a dict the prefixes' closed passes are kept in, keyed by their length
    -- streams over the same models and symbols may share one."""

    def __init__(self, models, ln_switch, B, L, closed_pass=R.posteriors_one, cache=None):
        assert B >= 1 and L >= 0
        self.models, self.ln_switch, self.B, self.L = models, float(ln_switch), int(B), int(L)
        self.K = len(models)
        self.closed_pass = closed_pass
        self.cache = {} if cache is None else cache
        self.sym = np.zeros(0, dtype=np.int64)
        self.next_b = 0      # the first block no launch has run for
        self.fwd = 0         # frames the forward pass has seen
        self.ready = 0       # frames delivered
        self.taken = 0
        self.rows = []       # delivered rows, in frame order
        self.status = 0
        self.frame = -1      # of the event
        self.closed = False
        self.log_prob = None
        self.launches = 0
        self.walked = 0      # frames the backward passes walked

    @property
    def fed(self):
        return len(self.sym)

    def window_end(self, b):
        return (b + 1) * self.B + self.L

    def ready_after(self, p):
        return ready_after(p, self.B, self.L)

    def prefix(self, n):
        """the closed pass on the first n symbols"""
        if n not in self.cache:
            self.cache[n] = self.closed_pass(self.models, self.sym[:n], self.ln_switch)
        return self.cache[n]

    def _event_frame(self, lo, hi):
        """the frame of the first event, known to lie in [lo, hi): the status of a prefix is 0 up to it and its status beyond"""
        while hi - lo > 1:  # invariant: prefix(lo) is clean, prefix(hi) is not
            mid = (lo + hi) // 2
            if self.prefix(mid)["status"] == 0:
                lo = mid
            else:
                hi = mid
        return lo

    def _launch(self, w, emit_hi):
        """one window: the forward pass over [fwd, w), the backward pass from w - 1 down to the first undelivered frame, the
        rows of [that frame, emit_hi)"""
        lo = self.next_b * self.B
        assert 0 <= lo < emit_hi <= w and w - lo <= self.B + self.L and w - self.fwd <= self.B + self.L
        self.launches += 1
        r = self.prefix(w)
        if r["status"] != 0:
            self.status = int(r["status"])
            self.frame = self._event_frame(self.fwd, w)
            return
        self.fwd = w
        self.walked += w - lo
        self.rows.extend(r["post"][lo:emit_hi])
        self.ready = emit_hi

    def take(self):
        first = self.taken
        rows = np.array(self.rows[self.taken:self.ready], dtype=np.float64).reshape(self.ready - self.taken, self.K)
        self.taken = self.ready
        return first, rows

    def feed(self, sym):
        if self.closed or self.status == 2:
            raise Refused()
        sym = np.asarray(sym, dtype=np.int64).ravel()
        self.sym = np.concatenate([self.sym, sym])
        if self.status == 1:  # accepted, counted, nothing else
            return self.take()
        while self.status == 0 and self.window_end(self.next_b) <= self.fed:
            self._launch(self.window_end(self.next_b), (self.next_b + 1) * self.B)
            if self.status == 0:
                self.next_b += 1
        if self.status == 2:  # (met by this feed: a session of status 2 takes no feed)
            raise BadSymbol(self.frame)
        return self.take()

    def close(self):
        if self.closed:
            raise Refused()
        raised = self.status == 2
        if self.status == 0 and self.fed > self.next_b * self.B:
            self._launch(self.fed, self.fed)
        self.closed = True
        if self.status == 0:
            self.log_prob = self.prefix(self.fed)["log_prob"]
        else:
            self.rows.extend(np.zeros((self.fed - self.ready, self.K)))
            self.ready = self.fed
            self.log_prob = NINF
            if self.status == 2 and not raised:
                raise BadSymbol(self.frame)
        return self.take()


def run(models, seq, ln_switch, B, L, feeds, closed_pass=R.posteriors_one, cache=None):
    """a stream fed seq in pieces of the lengths `feeds` and closed -> (the Stream, ready after each feed, every row delivered)"""
    s = Stream(models, ln_switch, B, L, closed_pass, cache)
    at, ready = 0, []
    for n in feeds:
        s.feed(seq[at:at + n])
        at += n
        ready.append(s.ready)
    s.close()
    return s, ready, np.array(s.rows, dtype=np.float64).reshape(len(s.rows), s.K)
