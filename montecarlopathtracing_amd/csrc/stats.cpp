// The device counters as the C API reports them (mcpt_stats) and as MCPT_PRINT_DIAG prints them.  Host only and HIP-free: the text the
// tests read is made here and nowhere else.
#include "stats.hpp"

#include <algorithm>
#include <cstdio>

using namespace mcpt;

void counters_to_stats(const DCounters& c, mcpt_stats* s, bool print_diag)
{
    s->rays_primary = c.rays_primary; s->rays_shadow = c.rays_shadow; s->rays_bounce = c.rays_bounce;
    s->node_visits = c.node_visits; s->tri_tests = c.tri_tests; s->shade_calls = c.shade_calls; s->samples = c.samples;
    s->shadow_skipped = c.shadow_skipped;
    s->dom_rays = c.trace_rays; s->dom_node_visits = c.trace_nodes; s->dom_tri_tests = c.trace_tris;
    if (print_diag) {
        const double tot = double(c.diag[TD_CYCLES + 0] + c.diag[TD_CYCLES + 1] + c.diag[TD_CYCLES + 2] + c.diag[TD_CYCLES + 3]);
        const double iters = double(c.diag[TD_ITERS + 2 * 0] + c.diag[TD_ITERS + 2 * 1] + c.diag[TD_ITERS + 2 * 2]);
        auto per = [](unsigned long long a, unsigned long long b) { return b ? double(a) / double(b) : 0.0; };
        std::fprintf(stderr, "trace diag: inner iters %llu lanes %.1f/64 | pre-test iters %llu lanes %.1f/64 | exact iters %llu lanes %.1f/64 | idle lanes/iter %.1f | "
                             "wave time: refill %.1f%% inner %.1f%% pre-test %.1f%% exact %.1f%% | cycles per iter: inner %.0f pre-test %.0f exact %.0f\n",
                     c.diag[TD_ITERS + 2 * 0], per(c.diag[TD_LANES + 2 * 0], c.diag[TD_ITERS + 2 * 0]), c.diag[TD_ITERS + 2 * 1], per(c.diag[TD_LANES + 2 * 1], c.diag[TD_ITERS + 2 * 1]), c.diag[TD_ITERS + 2 * 2], per(c.diag[TD_LANES + 2 * 2], c.diag[TD_ITERS + 2 * 2]), iters ? double(c.diag[TD_IDLE_LANES]) / iters : 0.0,
                     tot ? 100.0 * c.diag[TD_CYCLES + 0] / tot : 0.0, tot ? 100.0 * c.diag[TD_CYCLES + 1] / tot : 0.0, tot ? 100.0 * c.diag[TD_CYCLES + 2] / tot : 0.0, tot ? 100.0 * c.diag[TD_CYCLES + 3] / tot : 0.0,
                     per(c.diag[TD_CYCLES + 1], c.diag[TD_ITERS + 2 * 0]), per(c.diag[TD_CYCLES + 2], c.diag[TD_ITERS + 2 * 1]), per(c.diag[TD_CYCLES + 3], c.diag[TD_ITERS + 2 * 2]));
        std::fprintf(stderr, "k_wf_trace: %llu rays, %.3f nodes, %.3f triangles visited, %.3f exact tests per ray (%.1f %% of the visited triangles survive the pre-test)\n",
                     c.trace_rays, per(c.trace_nodes, c.trace_rays), per(c.trace_tris, c.trace_rays), per(c.trace_exact, c.trace_rays), 100.0 * per(c.trace_exact, c.trace_tris));
        std::fprintf(stderr, "rays deferred to the exact walk by k_wf_trace: %llu of %llu\n", c.deferred_rays, c.trace_rays);
#ifdef MCPT_POOL_DEBUG
        const PoolAccount& pa = c.dbg.account;
        if (pa.waves) {
            static const char* nm[5] = {"node", "leaf", "exact", "result", "shade"};
            const double life = double(pa.life);
            for (int i = 0; i < 5; i++)
                std::fprintf(stderr, "pool %-6s: %10llu steps, %5.1f lanes per step, %7.0f cycles per step, %5.1f %% of wave time\n", nm[i], pa.steps[i],
                             pa.steps[i] ? double(pa.lanes[i]) / pa.steps[i] : 0.0, pa.steps[i] ? double(pa.cycles[i]) / pa.steps[i] : 0.0, life ? 100.0 * pa.cycles[i] / life : 0.0);
            std::fprintf(stderr, "pool: %llu waves, %.0f cycles per wave, vote + claim + sleep %.1f %% of wave time, %llu sleeps, %llu steps that claimed nothing\n", pa.waves,
                         life / pa.waves, life ? 100.0 * pa.overhead / life : 0.0, pa.sleeps, pa.missed);
        }
        const PoolDebug& pd = c.dbg.pool;
        for (int i = 0; i < 4; i++) std::fprintf(stderr, "pool class %d: %llu steps, %.1f lanes per step (%.1f could before the claim)\n", i, pd.class_steps[i], pd.class_steps[i] ? double(pd.class_lanes[i]) / pd.class_steps[i] : 0.0, pd.class_steps[i] ? double(pd.class_want[i]) / pd.class_steps[i] : 0.0);
        std::fprintf(stderr, "pool: %llu sleeps, %llu steps that claimed nothing\n", pd.sleeps, pd.missed);
        std::fprintf(stderr, "pool debug: %llu launches, %llu slots in all, %llu consumed in %llu refill steps, %llu rays among them, %llu started, %llu slots retired, %llu tickets\n", pd.launches, pd.slots, pd.used, pd.refills, pd.ok, pd.started, pd.retired, pd.tickets);
#endif
        if (c.pre_wrong) {
            std::fprintf(stderr, "PRE-TEST SELF-CHECK: %llu rejected triangles are candidates by the exact test\n", c.pre_wrong);
            const PreCheckRecord& g = c.dbg.pre;
            std::fprintf(stderr, "  first: margins beta %.6g gamma %.6g alpha %.6g behind %.6g beyond %.6g clear %.6g | t32 %.9g |det| %.6g | t_k %.17g leader %.17g limit_f %.9g margin %.6g eta4 %.6g slot %.0f of %.0f\n"
                                 "  ray o %.17g %.17g %.17g d %.17g %.17g %.17g\n",
                         g.seen[0], g.seen[1], g.seen[2], g.seen[3], g.seen[4], g.seen[5], g.seen[6], g.seen[7], g.t_k, g.leader, g.limit_f, g.margin, g.eta4, g.slot, g.count,
                         g.o[0], g.o[1], g.o[2], g.d[0], g.d[1], g.d[2]);
        }
#ifdef MCPT_PRE_CHECK
        std::fprintf(stderr, "KERNARG CHECK: %llu of %llu trace launches read another WfArgs through the kernarg segment\n", c.kernarg_differ, c.kernarg_checked);
#endif
        if (c.finish_steps) std::fprintf(stderr, "finish diag: longest wave %llu steps, %.0f us alive, %.0f us of it in the ray walks (100 MHz ticks; maxima over waves and launches)\n",
                                    c.finish_steps, double(c.finish_life) / 100.0, double(c.finish_trace) / 100.0);
        const double lt = double(c.logic_cycles[0] + c.logic_cycles[1] + c.logic_cycles[2]);
        std::fprintf(stderr, "logic diag: resolve %.1f%% compaction %.1f%% shade %.1f%% | cycles per wave: %.0f / %.0f / %.0f (waves %llu)\n",
                     lt ? 100.0 * c.logic_cycles[0] / lt : 0.0, lt ? 100.0 * c.logic_cycles[1] / lt : 0.0, lt ? 100.0 * c.logic_cycles[2] / lt : 0.0,
                     c.logic_waves ? double(c.logic_cycles[0]) / c.logic_waves : 0.0, c.logic_waves ? double(c.logic_cycles[1]) / c.logic_waves : 0.0, c.logic_waves ? double(c.logic_cycles[2]) / c.logic_waves : 0.0, c.logic_waves);
    }
}

void add_counts(mcpt_stats& a, const mcpt_stats& b)
{
    a.rays_primary += b.rays_primary; a.rays_shadow += b.rays_shadow; a.rays_bounce += b.rays_bounce;
    a.node_visits += b.node_visits; a.tri_tests += b.tri_tests; a.shade_calls += b.shade_calls;
    a.samples += b.samples; a.shadow_skipped += b.shadow_skipped;
    a.dom_rays += b.dom_rays; a.dom_node_visits += b.dom_node_visits; a.dom_tri_tests += b.dom_tri_tests;
    a.launches += b.launches;
    a.max_depth = std::max(a.max_depth, b.max_depth);
}

void add_piece(mcpt_stats& a, const mcpt_stats& piece)
{
    add_counts(a, piece);
    a.ms_trace += piece.ms_trace;
    a.ms_total += piece.ms_total;
}
