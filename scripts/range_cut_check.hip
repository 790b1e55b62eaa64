// Host-only check that tbx_range_step / tbx_each_range (csrc/tbx_common.hpp) cut the envs of every planner query exactly as the five
// copies of the rule did before they became one function.  The five "before_*" functions below are those copies, kept verbatim from
// the commit before (`Engine` below stands in for tbx_engine).  No GPU: build the host side with the sanitizers and run it.
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined scripts/range_cut_check.hip -o /tmp/range_cut_check \
//         && /tmp/range_cut_check
//
// Grid: n in {1, 2, 5, 24, 700, 4 096, 65 536, 2^20} x the four games x both search_lanes() x the smallest, a middling and the
// largest valid row of every query (and the budget of per-env rows the host has not seen) x TBX_OPT_BEAM_RANGE_ENVS in {0, 1, 7, n}.
// Prints the cells compared per query and exits 1 on the first difference.
#include <cstdio>
#include <utility>
#include <vector>

#include "../toybox_amd/csrc/tbx_common.hpp"

using Ranges = std::vector<std::pair<int, int>>;

// ---- the commit before: tbx_common.hpp
template <class F>
void before_search_launches(int n, long long units_per_env, long long leaf_frames_per_env, F&& f)
{
    long long step = TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH / leaf_frames_per_env;
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (step < 1) step = 1;
    for (long long e0 = 0; e0 < n; e0 += step) f((int)e0, (int)(n - e0 < step ? n - e0 : step));
}
template <class F>
int before_search_samples_launches(int n, long long units_per_env, long long leaf_frames_per_env, long long budget, F&& f)
{
    long long step = budget / leaf_frames_per_env;
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (step < 1) step = 1;
    int launches = 0;
    for (long long e0 = 0; e0 < n; e0 += step, launches++) f((int)e0, (int)(n - e0 < step ? n - e0 : step));
    return launches;
}
// ---- the commit before: the ladders of lookahead_beam, lookahead_evolve and lookahead_beam_samples (engine.hip) and their loop
struct Engine {
    int n, beam_range_envs, game;
};
static long long before_beam_step(const Engine* e, long long units_per_env, size_t bytes_per_env, long long frames)
{
    long long step = TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH / (units_per_env * frames);
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (step > (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env)) step = (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env);
    if (e->beam_range_envs > 0 && step > e->beam_range_envs) step = e->beam_range_envs;
    if (step > e->n) step = e->n;
    if (step < 1) step = 1;
    return step;
}
struct Bounds {
    long long frames, leaves;
};
static long long before_evolve_step(const Engine* e, long long units_per_env, size_t bytes_per_env, const Bounds& b)
{
    long long step = TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH / (units_per_env * b.frames);
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (step > (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env)) step = (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env);
    if (e->beam_range_envs > 0 && step > e->beam_range_envs) step = e->beam_range_envs;
    if (step > e->n) step = e->n;
    if (step < 1) step = 1;
    return step;
}
static long long before_beam_samples_step(const Engine* e, int lanes, long long units_per_env, size_t bytes_per_env, const Bounds& b)
{
    long long step = tbx_search_samples_budget(e->game, lanes) / (b.leaves * b.frames);
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (step > (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env)) step = (long long)(TBX_BEAM_SCRATCH_BYTES / bytes_per_env);
    if (e->beam_range_envs > 0 && step > e->beam_range_envs) step = e->beam_range_envs;
    if (step > e->n) step = e->n;
    if (step < 1) step = 1;
    return step;
}
static Ranges before_ladder_ranges(const Engine* e, long long step, int& ranges_out)
{
    Ranges r;
    int ranges = 0;
    for (long long env0 = 0; env0 < e->n; env0 += step, ranges++) {
        const int envs = (int)(e->n - env0 < step ? e->n - env0 : step);
        r.push_back({(int)env0, envs});
    }
    ranges_out = ranges;
    return r;
}

// ---- the comparison
static long long cells[6];
static const char* const NAMES[6] = {"153 search", "154 samples", "155 search over samples", "156 beam", "157 beam over samples", "158 evolve"};

static bool same(int q, const char* what, int n, int game, int lanes, long long a, long long b)
{
    if (a == b) return true;
    printf("DIFFERENT %s, %s: n %d game %d lanes %d: before %lld, now %lld\n", NAMES[q], what, n, game, lanes, a, b);
    return false;
}
static bool same_ranges(int q, int n, int game, int lanes, const Ranges& a, const Ranges& b)
{
    if (!same(q, "ranges", n, game, lanes, (long long)a.size(), (long long)b.size())) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!same(q, "first_env", n, game, lanes, a[i].first, b[i].first) || !same(q, "envs", n, game, lanes, a[i].second, b[i].second)) return false;
    cells[q]++;
    return true;
}
// a search-shaped query: no step on the old side, so the ranges and their count
static bool check_launches(int q, int n, int game, int lanes, long long budget, bool own_budget, long long units_per_env, long long leaf_frames_per_env)
{
    Ranges before, now;
    int count_before = -1;
    if (own_budget) count_before = before_search_samples_launches(n, units_per_env, leaf_frames_per_env, budget, [&](int e0, int envs) { before.push_back({e0, envs}); });
    else before_search_launches(n, units_per_env, leaf_frames_per_env, [&](int e0, int envs) { before.push_back({e0, envs}); });
    const int count = tbx_each_range(n, tbx_range_step(n, budget, leaf_frames_per_env, units_per_env), [&](int e0, int envs) { now.push_back({e0, envs}); });
    if (own_budget && !same(q, "launches", n, game, lanes, count_before, count)) return false;
    return same(q, "launches", n, game, lanes, (long long)before.size(), count) && same_ranges(q, n, game, lanes, before, now);
}
// a ladder: the step, the ranges and their count
static bool check_ladder(int q, const Engine& e, int game, int lanes, long long step_before, long long budget, long long leaf_frames_per_env, long long units_per_env,
                         size_t bytes_per_env)
{
    const long long step = tbx_range_step(e.n, budget, leaf_frames_per_env, units_per_env, bytes_per_env, e.beam_range_envs);
    if (!same(q, "step", e.n, game, lanes, step_before, step)) return false;
    int count_before = 0;
    const Ranges before = before_ladder_ranges(&e, step_before, count_before);
    Ranges now;
    const int count = tbx_each_range(e.n, step, [&](int e0, int envs) { now.push_back({e0, envs}); });
    return same(q, "range count", e.n, game, lanes, count_before, count) && same_ranges(q, e.n, game, lanes, before, now);
}

int main()
{
    const int ns[] = {1, 2, 5, 24, 700, 4096, 65536, 1 << 20};
    const int games[] = {TBX_GAME_BREAKOUT, TBX_GAME_SPACE_INVADERS, TBX_GAME_AMIDAR, TBX_GAME_GRIDWORLD};
    bool ok = true;
    for (int n : ns)
        for (int game : games)
            for (int lanes : {64, 1}) {
                const int L = tbx_legal_count(game), top = tbx_plan_max_depth(game);
                int deepest = 1;                              // the deepest full search: L^depth <= TBX_LOOKAHEAD_MAX_PLANS
                while (tbx_plan_count(game, deepest + 1) <= (uint64_t)TBX_LOOKAHEAD_MAX_PLANS) deepest++;
                const long long budget = tbx_search_samples_budget(game, lanes);
                // 153: {frames, depth}; the last row is what per-env rows are budgeted as
                const long long search_rows[4][2] = {{1, (long long)tbx_plan_count(game, 1)}, {64, (long long)tbx_plan_count(game, 3)},
                                                     {TBX_LOOKAHEAD_MAX_FRAMES, (long long)tbx_plan_count(game, deepest)}, {TBX_LOOKAHEAD_MAX_FRAMES, TBX_LOOKAHEAD_MAX_PLANS}};
                for (auto& r : search_rows) {
                    const int chunks = tbx_search_chunks(n, L, r[1] / L, lanes);
                    ok = ok && check_launches(0, n, game, lanes, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, false, (long long)L * chunks, r[1] * r[0]);
                }
                // 154: {frames, samples}
                const long long sample_rows[3][2] = {{1, 1}, {64, 16}, {TBX_LOOKAHEAD_MAX_FRAMES, TBX_LOOKAHEAD_MAX_SAMPLES}};
                for (auto& r : sample_rows) {
                    const int chunks = tbx_search_chunks(n, L, r[1], lanes);
                    ok = ok && check_launches(1, n, game, lanes, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, false, (long long)L * chunks, r[1] * r[0]);
                }
                // 155: {frames, plans, samples}, plans x samples <= TBX_LOOKAHEAD_MAX_LEAVES; the last row: per-env rows
                const long long deepest_plans = (long long)tbx_plan_count(game, deepest);
                const long long ss_rows[4][3] = {{1, L, 1}, {64, (long long)tbx_plan_count(game, 2), 16}, {TBX_LOOKAHEAD_MAX_FRAMES, deepest_plans, TBX_LOOKAHEAD_MAX_LEAVES / deepest_plans},
                                                 {TBX_LOOKAHEAD_MAX_FRAMES, TBX_LOOKAHEAD_MAX_PLANS, TBX_LOOKAHEAD_MAX_LEAVES / TBX_LOOKAHEAD_MAX_PLANS}};
                for (int i = 0; i < 4; i++) {
                    const long long* r = ss_rows[i];
                    const int chunks = tbx_search_chunks(n, L, r[1] / L, lanes);
                    const long long leaves = i == 3 ? (long long)TBX_LOOKAHEAD_MAX_LEAVES : r[1] * r[2];
                    ok = ok && check_launches(2, n, game, lanes, budget, true, (long long)L * chunks, leaves * r[0]);
                }
                for (int range_envs : {0, 1, 7, n}) {
                    const Engine e{n, range_envs, game};
                    // 156: {frames, width}
                    const long long beam_rows[3][2] = {{1, 1}, {64, 4}, {TBX_LOOKAHEAD_MAX_FRAMES, TBX_BEAM_MAX_WIDTH}};
                    for (auto& r : beam_rows) {
                        const long long frames = r[0];
                        const int width = (int)r[1];
                        const long long units_per_env = (long long)L * width * L;
                        const size_t bytes_per_env = (size_t)units_per_env * sizeof(TbxBeamCand) + 2 * (size_t)L * width * sizeof(uint32_t);
                        ok = ok && check_ladder(3, e, game, lanes, before_beam_step(&e, units_per_env, bytes_per_env, frames), TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH,
                                                units_per_env * frames, units_per_env, bytes_per_env);
                    }
                    // 157: {frames, depth, width, samples}; the last row: per-env rows the host has not seen
                    const int cap = TBX_LOOKAHEAD_MAX_LEAVES / (L * TBX_BEAM_MAX_WIDTH * L);
                    const long long bs_rows[4][4] = {{1, 1, 1, 1}, {64, 4, 4, 16}, {TBX_LOOKAHEAD_MAX_FRAMES, top, TBX_BEAM_MAX_WIDTH, cap},
                                                     {TBX_LOOKAHEAD_MAX_FRAMES, top, TBX_BEAM_MAX_WIDTH, TBX_LOOKAHEAD_MAX_SAMPLES}};
                    for (int i = 0; i < 4; i++) {
                        const long long* r = bs_rows[i];
                        const int depth = (int)r[1], width = (int)r[2];
                        Bounds b{r[0], (long long)L * tbx_beam_kept(L, width, depth - 1) * (depth == 1 ? 1 : L) * r[3]};
                        if (i == 3) b.leaves = TBX_LOOKAHEAD_MAX_LEAVES;
                        const long long units_per_env = (long long)L * width * L;
                        const size_t beam_bytes_per_env = 2 * (size_t)L * width * sizeof(uint32_t), rec_bytes = 9 * sizeof(long long);
                        const size_t bytes_per_env = (size_t)units_per_env * rec_bytes + beam_bytes_per_env;
                        ok = ok && check_ladder(4, e, game, lanes, before_beam_samples_step(&e, lanes, units_per_env, bytes_per_env, b), budget, b.leaves * b.frames,
                                                units_per_env, bytes_per_env);
                    }
                    // 158: {frames, population}
                    const long long evolve_rows[3][2] = {{1, 1}, {64, 64}, {TBX_LOOKAHEAD_MAX_FRAMES, TBX_EVOLVE_MAX_POPULATION}};
                    for (auto& r : evolve_rows) {
                        const Bounds b{r[0], 0};
                        const long long units_per_env = (long long)L * r[1];
                        const size_t bytes_per_env = (size_t)units_per_env * (sizeof(TbxBeamCand) + sizeof(uint32_t));
                        ok = ok && check_ladder(5, e, game, lanes, before_evolve_step(&e, units_per_env, bytes_per_env, b), TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH,
                                                units_per_env * b.frames, units_per_env, bytes_per_env);
                    }
                }
            }
    long long all = 0;
    for (int q = 0; q < 6; q++) {
        printf("%-24s %5lld cells equal\n", NAMES[q], cells[q]);
        all += cells[q];
    }
    printf("%s: %lld cells\n", ok ? "every step and every (first_env, envs) list equal" : "DIFFERENCES", all);
    return ok ? 0 : 1;
}
