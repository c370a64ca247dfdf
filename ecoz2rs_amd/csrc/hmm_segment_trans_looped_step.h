// hmm_segment_trans_looped_step.h -- a frame of the looped body of the joint Viterbi under class-to-class prices (DESIGN.md
// 4.8.8, "The looped body"), written once for its two kernels (hmm_segment_trans_looped.hip: a closed stream, and one block of
// an open one): the turn of a served slot before the frame's barrier, its turn after it, and the frame that has no
// predecessor.  The arithmetic is hmm_segment_trans_step.h's -- chain_max_exit and source_walk, called as the resident stream
// kernel calls them -- so every d, psi, src, x and E has the resident body's bits.
// What outlives a turn lives in LDS, indexed by the composite state and touched by that state's own lane alone (LoopedCarry): a
// register file as long as the wave's turns, which needs no fence and no barrier of its own.
// Device code only.  Internal.
#pragma once
#include "hmm_segment_common.h"
#include "hmm_segment_trans_step.h"

namespace e2hmm {

namespace {

struct LoopedCarry {
    double* d;     // [sumN] d of the state: of the previous frame before the frame's second pass, of this frame after it
    double* best;  // [sumN] the in-class maximum of the frame, from the first pass to the second
    int* arg;      // [sumN] and its state
};

// the tables' rows of one frame: psi (sumN), src (K), x (K), E (K)
struct LoopedRows {
    u16* psi;
    u16* src;
    u16* xs;
    double* Es;
};

// what the turns of a slot share: the lane of slot sl and the slot's chain route (wave-uniform)
struct LoopedLane {
    SegLaneDev L;
    bool act, head;  // the lane has a state; it posts and stores for its class
    int c, k;        // composite index, class (0 for a lane without a state: its reads stay in bounds)
};

__device__ __forceinline__ LoopedLane looped_lane(const SegPlanDev& pl, int sl, int lane)
{
    LoopedLane q;
    q.L = pl.lanes[sl * 64 + lane];
    q.act = q.L.cls >= 0;
    q.head = q.act && q.L.j == 0;
    q.c = q.act ? q.L.comp : 0;
    q.k = q.act ? q.L.cls : 0;
    return q;
}

// the frame without a predecessor (the absolute frame 0): d = lpi + b
__device__ __forceinline__ void looped_first_turn(const SegPlanDev& pl, int sl, int lane, int o, const double* lpi, const double* lB,
                                                  const LoopedCarry& cy)
{
    const LoopedLane q = looped_lane(pl, sl, lane);
    if (q.act) cy.d[q.c] = lpi[q.c] + lB[(size_t)q.c * pl.M + o];
}

// before the barrier: the in-class chain over d of the previous frame, and on the way the class's exit.  The head lane posts E
// to Et[k] and stores x and E; best and arg wait in LDS for the second pass.
__device__ __forceinline__ void looped_exit_turn(const SegPlanDev& pl, int sl, int lane, const double* lA, const LoopedCarry& cy,
                                                 double* Et, const LoopedRows& row)
{
    const LoopedLane q = looped_lane(pl, sl, lane);
    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
    const double d = q.act ? cy.d[q.c] : -__builtin_inf();  // (a lane without a state is kept at -inf, as in the resident body)
    const ChainExit ce = chain_max_exit(d, lA + q.L.a_at + q.L.j, q.L.N, q.L.seg, maxN, single);
    if (q.head) {
        Et[q.k] = ce.E;
        row.xs[q.k] = (u16)ce.x;
        row.Es[q.k] = ce.E;
    }
    if (q.act) {
        cy.best[q.c] = ce.best;
        cy.arg[q.c] = ce.arg;
    }
}

// after the barrier: the walk over the K sources, ENTER against the chain's maximum (a tie stays in the class), d = best + b.
// The emission is requested first: the walk hides it.
__device__ __forceinline__ void looped_enter_turn(const SegPlanDev& pl, int sl, int lane, int o, const double* lpi, const double* lB,
                                                  const double* ltT, const LoopedCarry& cy, const double* Et, const LoopedRows& row)
{
    const LoopedLane q = looped_lane(pl, sl, lane);
    const double bq = q.act ? lB[(size_t)q.c * pl.M + o] : 0.0;
    const double lpij = q.act ? lpi[q.c] : -__builtin_inf();
    const Source sw = source_walk(Et, ltT + (size_t)q.k * pl.K, pl.K);
    if (!q.act) return;
    double best = cy.best[q.c];
    int arg = cy.arg[q.c];
    const double xe = sw.base + lpij;
    if (xe > best) {  // (a tie stays in the class)
        best = xe;
        arg = ENTER;
    }
    cy.d[q.c] = best + bq;
    row.psi[q.c] = (u16)arg;
    if (q.head) row.src[q.k] = (u16)sw.from;
}

}  // namespace

}  // namespace e2hmm
