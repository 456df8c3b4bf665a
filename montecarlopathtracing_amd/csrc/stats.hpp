// stats.cpp: the device counters as mcpt_stats and as the MCPT_PRINT_DIAG text.  Host only, no HIP.
#pragma once
#include "../../include/mcpt.h"
#include "device_scene.hpp"

#pragma GCC visibility push(hidden)
void counters_to_stats(const mcpt::DCounters& c, mcpt_stats* s, bool print_diag);
// a += b for every counter of b (max_depth: the larger); ms_trace and ms_total are the caller's to combine
void add_counts(mcpt_stats& a, const mcpt_stats& b);
// the statistics of one piece of a call (a pass, a shutter step) added to the call's: add_counts and the two times, which follow one another
void add_piece(mcpt_stats& a, const mcpt_stats& piece);
#pragma GCC visibility pop
