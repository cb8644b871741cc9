// tests/fast_chunks_probe.cpp -- C entry points over the planner's fast-tier chunk arithmetic (uhc_plan.cpp) for tests/test_fast_chunks_cpu.py: host compiler only.
#include <cstdlib>
#include <cstring>

#include "uhc_plan.h"

#define PROBE extern "C" __attribute__((visibility("default")))

// out: chunk, n_chunks, grid, prod_total
PROBE void uhc_fc_plan(int n_substeps, int chunk, int n_env, int* out) {
    const FastChunks f = plan_fast_chunks(n_substeps, chunk, n_env);
    out[0] = f.chunk; out[1] = f.n_chunks; out[2] = f.grid; out[3] = f.prod_total;
}
PROBE void uhc_fc_range(int n_substeps, int chunk, int n_env, int c, int* lo_hi) {
    const FastChunks f = plan_fast_chunks(n_substeps, chunk, n_env);
    fast_chunk_range(f, n_substeps, c, lo_hi, lo_hi + 1);
}
PROBE int uhc_fc_default(int knob, int n_substeps, int n_env, int n_cu, int lds_bytes_fast) {
    return default_fast_chunk(knob, n_substeps, n_env, n_cu, (size_t)lds_bytes_fast);
}
// value == NULL: the variable is not set.  out: BatchKnobs::fast_chunk, fast_chunk_bad
PROBE void uhc_fc_knob(const char* value, int* out) {
    if (value) setenv("UHC_FAST_CHUNK", value, 1); else unsetenv("UHC_FAST_CHUNK");
    const BatchKnobs k = read_knobs();
    unsetenv("UHC_FAST_CHUNK");
    out[0] = k.fast_chunk; out[1] = k.fast_chunk_bad ? 1 : 0;
}
// the sticky step's view: StickyInputs with everything but the batch size, the chip and the chunk knob at zero.  out as uhc_fc_plan
PROBE void uhc_fc_sticky(int n_env, int n_cu, int lds_bytes_fast, int fast_chunk, int n_substeps, int* out) {
    StickyInputs in{};
    in.n_env = n_env; in.n_cu = n_cu; in.lds_bytes_fast = (size_t)lds_bytes_fast; in.last_tier = 4; in.q2_div = 1; in.q2_wait_min = 16; in.q2_max = 256; in.q3_max = 32; in.q4_max = 16;
    in.fast_chunk = fast_chunk; in.n_substeps = n_substeps;
    const FastChunks f = plan_sticky_step(in).fast;
    out[0] = f.chunk; out[1] = f.n_chunks; out[2] = f.grid; out[3] = f.prod_total;
}
