// Stand-alone driver of stats.cpp for test_stats_cpu.py: a DCounters whose 64-bit word i holds i + 1, through counters_to_stats with the
// diagnostics on, then the mcpt_stats fields it filled.  Everything goes to stderr, in order.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../montecarlopathtracing_amd/csrc/stats.hpp"

int main()
{
    unsigned long long words[sizeof(mcpt::DCounters) / sizeof(unsigned long long)];
    for (size_t i = 0; i < sizeof words / sizeof words[0]; i++) words[i] = i + 1;
    mcpt::DCounters c;
    std::memcpy(&c, words, sizeof c);
    mcpt_stats s;
    std::memset(&s, 0, sizeof s);
    counters_to_stats(c, &s, true);
    std::fprintf(stderr, "stats: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                         " | %.1f %.1f %d %d\n",
                 s.rays_primary, s.rays_shadow, s.rays_bounce, s.node_visits, s.tri_tests, s.shade_calls, s.samples, s.shadow_skipped, s.dom_rays,
                 s.dom_node_visits, s.dom_tri_tests, s.ms_trace, s.ms_total, s.launches, s.max_depth);
    mcpt_stats t = s;
    t.max_depth = 7;
    add_counts(t, s);
    std::fprintf(stderr, "sum: %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %d\n", t.rays_primary, t.samples, t.dom_tri_tests, t.launches, t.max_depth);
    return 0;
}
