// sgo_policy.h -- what sgo_optimize_gn keeps about its multigrid hierarchy and the decisions one call takes from it, apart from the GPU
// work they drive (optimize_gn, sgo_solve.cpp).  Host-only, every rule and constant sgo_rules.h's; unit-tested in tests/cpp/rules_unit.cpp.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "sgo_rules.h"

namespace sgo {

// What the resident graph's hierarchy has taught so far: lives as long as the graph or the hierarchy, as each operation below says.
struct HierarchyState {
  int best = 0;                  // fewest PCG iterations seen with the current hierarchy (0: none yet), kept across calls
  int agg_best = 0;              // the fewest PCG iterations a fresh solve behind this aggregation has taken
  // PCG iterations a unit of movement costs this graph's solves, learned from the kept solves (C4: ~1000, 50k / 250k: ~4000-8000)
  double lag_slope = rules::kLagSlopeStart;
  bool lag_slope_seen = false;
  int lag_n = 0;                 // rows of the graph the slope was learned on
  int probe_k = 0;               // progress probe of the kept solves (PcgScalars::probe_k / probe_max), from the last fresh solve
  double probe_max = 0.0;
  bool ref_valid = false;        // d_dref holds the blocks of the resident coarse operators
  bool agg_ref_valid = false;    // d_dref_agg holds the blocks the hierarchy was aggregated from
  bool agg_rule_off = false;     // a trial was lost on this graph: the re-aggregation rule does not fire again before the next set-up
  bool no_filter = false;        // this graph's hierarchy rebuilds keep the tentative transfer where the smoothed one is refused
  double theta_scale = 1.0;      // strength thresholds of the next hierarchy build, as a factor (halved when a first solve stalls)

  // a new graph is set (the slope and the probe record are carried over a graph of about the same size: begin_call)
  void new_graph() { ref_valid = agg_ref_valid = agg_rule_off = no_filter = false; theta_scale = 1.0; }
  // the solves from here on have another right-hand side (an incremental update): their first one sets a new reference
  void new_rhs() { best = 0; }
  // a hierarchy was (re)made (build_amg): its counts and the reference of its coarse operators start over
  void new_hierarchy() { best = agg_best = 0; ref_valid = false; }
  // the hierarchy a trial replaced is back: its coarse operators are two iterations old, the blocks it was aggregated from unknown
  void reverted() { new_hierarchy(); probe_max = 0.0; agg_ref_valid = false; }
  // sgo_optimize_gn begins: the call's first solve refreshes; another graph's sensitivity is not known yet
  void begin_call(int n, double slope_hook) {
    if (lag_n == 0 || std::abs(n - lag_n) > lag_n / 10) { lag_slope = rules::kLagSlopeStart; lag_slope_seen = false; }
    lag_n = n;
    if (slope_hook > 0.0) { lag_slope = slope_hook; lag_slope_seen = false; }   // test hook (SGO_AMG_LAG_SLOPE): what every call starts from
    ref_valid = false;   // (the call's first solve refreshes)
    probe_max = 0.0;
    if (probe_k < 4) probe_k = 6;
  }
};

// One finished solve behind the hierarchy, as CallPolicy::record reads it.
struct SolveRecord {
  int it, iter;                    // Gauss-Newton iteration, PCG iterations
  double tol0, tolk;               // the call's relative tolerance and the one the solve stopped at (equal_tolerance_count)
  bool kept, interrupted, floor;   // behind kept coarse operators; those interrupted and carried on; accepted at the floating-point floor
  double moved;                    // the blocks' movement against the coarse operators' reference (relative)
  int probe_k;                     // the solve's progress probe (PcgScalars::probe_k / probe_rel)
  double probe_rel;
  bool trial_parked;               // the hierarchy a trial replaced is still parked (what a revert puts back)
  const double* agg_moved;         // [3] movement since the aggregation (k_diag_change's sums; nullptr: not measured)
  int n;                           // rows
};

// The decisions of ONE sgo_optimize_gn call: caps, rebuilds, the re-aggregation trial, staleness, and the call's note.
struct CallPolicy {
  enum Action { kNothing, kRebuildNext, kRevertTrial };
  enum Trial { kNoTrial, kTrialPending, kTrialJudging };   // pending: the trial's rebuild is next; judging: its first solves

  int iters, max_rebuilds, rebuild_cost;   // (max_rebuilds: a cap on the set-ups redone inside one call, against thrashing)
  int rebuilds = 0;
  bool rebuild_next;
  Trial trial = kNoTrial;
  int trial_old = 0, trial_best = 0, trial_seen = 0;
  int fresh_pcg = 0;      // the count of the last solve behind freshly made coarse operators
  int call_best = 0;      // the fewest (equal-tolerance) iterations a fresh solve of this call has taken
  int kept_solves = 0;
  int floor_solves = 0;   // solves accepted at the floating-point floor of their system
  std::string agg_note;   // what the re-aggregation rule did (sgo_solver_description)

  CallPolicy(int iters_, int rebuild_cost_, bool rebuild_first)
      : iters(iters_), max_rebuilds(rules::max_rebuilds(iters_)), rebuild_cost(rebuild_cost_), rebuild_next(rebuild_first) {}

  bool can_rebuild() const { return rebuilds < max_rebuilds; }
  bool last_rebuild() const { return rebuilds + 1 >= max_rebuilds; }

  // The iteration cap of the next solve (0: none): the bail-out cap of a hierarchy that has solved before; one that never has gets
  // first_cap (the hardest first solves seen take 200-350: C4 from a dead-reckoned start), then is redone (abandon).
  int solve_cap(const HierarchyState& g, bool has_amg, int first_cap) const {
    int cap = (has_amg && g.best > 0 && can_rebuild() && !rebuild_next) ? rules::bail_out_cap(g.best) : 0;
    if (has_amg && g.best == 0 && can_rebuild() && g.theta_scale > 0.2) cap = first_cap;
    return cap;
  }
  int lag_cap() const { return rules::lag_cap(fresh_pcg); }
  // ... of a kept solve's continuation after its operators were refreshed at iteration `at`
  int continue_cap(const HierarchyState& g, int at) const { return (g.best > 0 && can_rebuild()) ? rules::bail_out_cap(g.best) + at : 0; }

  // A solve ran into its cap: a hierarchy that never solved anything keeps tentative transfers where it FILTERED (sgo_amg_host.h), or is
  // coarsened more aggressively; the call's LAST rebuild keeps them anyway -- they go stale gracefully (190 -> 240 iterations, where a
  // stale filtered one can grind on to pcg_maxit).  One that HAS solved is stale: the rebuild filters by the current values.
  void abandon(HierarchyState& g, bool filtered) const {
    if (g.best == 0 && filtered) g.no_filter = true;
    else if (g.best == 0) g.theta_scale *= 0.5;
    if (last_rebuild()) g.no_filter = true;
  }

  // A rebuild happened: another hierarchy, whose first solve sets the call's reference (a pending trial is judged from here on).
  void rebuilt() {
    if (trial == kTrialPending) trial = kTrialJudging;
    ++rebuilds;
    call_best = 0;   // (another hierarchy: its first solve sets the reference)
    rebuild_next = false;
  }
  // The trial's set-up did not come about: the parked hierarchy is back, the rule off for this graph, the call goes on as if untried.
  void trial_failed(HierarchyState& g, const std::string& why) {
    g.reverted();
    g.agg_rule_off = true;
    trial = kNoTrial;
    rebuild_next = false;
    agg_note = "a re-aggregation was attempted in the last sgo_optimize_gn and its set-up failed" + (why.empty() ? std::string() : " (" + why + ")") +
               ": the previous hierarchy stays";
  }

  // A solve behind kept operators was interrupted (progress probe or cap) at a movement of `moved` (rules::lag_slope_after_interrupt).
  void kept_interrupted(HierarchyState& g, double moved) const { g.lag_slope = rules::lag_slope_after_interrupt(g.lag_slope, moved); g.lag_slope_seen = true; }

  // A finished solve (no breakdown) behind the hierarchy: what it teaches and what the driver does next (`log`: [sgo] lines, or nullptr).
  Action record(HierarchyState& g, const SolveRecord& s, std::FILE* log) {
    const int eq_iter = rules::equal_tolerance_count(s.iter, s.tol0, s.tolk);
    if (s.interrupted || s.floor) return kNothing;
    if (s.kept) {
      // judged against the last fresh solve only (too slow: the next solve refreshes whatever moved); every one teaches the slope
      ++kept_solves;
      if (rules::kept_solve_too_slow(eq_iter, fresh_pcg)) g.ref_valid = false;
      g.lag_slope = rules::lag_slope_after_kept(g.lag_slope, g.lag_slope_seen, eq_iter - fresh_pcg, s.moved);
      g.lag_slope_seen = true;
      return kNothing;
    }
    Action act = kNothing;
    fresh_pcg = eq_iter;
    g.lag_slope = rules::lag_slope_after_fresh(g.lag_slope);   // (a high slope is re-examined in time)
    if (trial == kTrialJudging) {
      // the re-made hierarchy's better count of its first two (fresh, warm-started) solves against the old one's first solve of the
      // call (cold): 22 / 24 against 33 keeps it; 42 / 38 against 27 puts the old one back
      trial_best = trial_seen == 0 ? eq_iter : std::min(trial_best, eq_iter);
      if (++trial_seen == 2) {
        trial = kNoTrial;
        if (rules::trial_reverts(trial_best, trial_old)) {
          act = kRevertTrial;
          if (s.trial_parked) g.reverted();
          g.agg_rule_off = true;
          call_best = fresh_pcg = 0;
          rebuild_next = false;
          agg_note = "a re-aggregated hierarchy was tried in the last sgo_optimize_gn and dropped (" + std::to_string(trial_best) + " PCG iterations against the old one's " + std::to_string(trial_old) + ")";
        }
      }
    }
    if (g.agg_best == 0 || eq_iter < g.agg_best) g.agg_best = eq_iter;   // (an incremental update resets best, not this)
    // the progress probe of the solves that keep these operators: iteration fresh / 3 (at least 4), half a decade of slack
    if (s.probe_k > 0 && s.iter >= s.probe_k && s.probe_rel > 0.0) g.probe_max = 10.0 * s.probe_rel;
    else if (s.probe_k > 0) g.probe_max = 0.0;
    const int k_new = rules::probe_iteration(s.iter);
    if (s.probe_k < 4 || std::abs(k_new - s.probe_k) > 1) {   // (the record was taken at another iteration: the next fresh solve records anew)
      g.probe_k = k_new;
      g.probe_max = 0.0;
    }
    if (g.best == 0 || eq_iter < g.best) g.best = eq_iter;
    // Staleness by counts, against the best of THIS call: no clocks, so that every rank decides alike.
    if (call_best == 0 || eq_iter < call_best) call_best = eq_iter;
    if (can_rebuild() && rules::staleness(eq_iter, call_best, iters - s.it - 1, rebuild_cost).rebuild()) rebuild_next = true;
    // The aggregation's own staleness, across calls: blocks moved far since the hierarchy was aggregated and this call's first
    // solve visibly above the aggregation's best -- the set-up is redone as a TRIAL.
    if (s.agg_moved) {
      const double* v = s.agg_moved;
      if (log) std::fprintf(log, "[sgo] since the aggregation: blocks moved by %.2f %%, %.0f rows by a quarter; first solve %d, best of this aggregation %d\n", v[1] > 0 ? 100.0 * v[0] / v[1] : 0.0, v[2], eq_iter, g.agg_best);
      if (rules::reaggregate(rules::moved_far(v[0], v[1], v[2], s.n), g.agg_rule_off, iters - s.it, g.agg_best, eq_iter, rebuilds, max_rebuilds, rebuild_next)) {
        rebuild_next = true;
        trial = kTrialPending;
        trial_old = eq_iter;
        char nb[160];
        std::snprintf(nb, sizeof nb, "hierarchy re-aggregated in the last sgo_optimize_gn (the blocks had moved by %.0f %% since it was made)", 100.0 * v[0] / v[1]);
        agg_note = nb;
        if (log)
          std::fprintf(log, "[sgo] the blocks have moved by %.1f %% (%.0f rows by a quarter) since the hierarchy was aggregated, first solve %d against its best %d: rebuild\n",
                       100.0 * v[0] / v[1], v[2], eq_iter, g.agg_best);
      }
    }
    return act == kNothing && rebuild_next ? kRebuildNext : act;
  }

  // What sgo_solver_description says about the call that `done` Gauss-Newton iterations ended.
  std::string note(int done) const {
    std::string s = kept_solves > 0 ? "last sgo_optimize_gn: " + std::to_string(kept_solves) + " of " + std::to_string(done) + " solves kept the coarse operators of the one before" : "";
    if (!agg_note.empty()) s += (s.empty() ? "" : "; ") + agg_note;
    if (floor_solves > 0)
      s += std::string(s.empty() ? "last sgo_optimize_gn: " : "; ") + std::to_string(floor_solves) +
           " solve(s) stopped at the floating-point floor of their system (Jacobi-scaled backward error <= 1e-12 without reaching pcg_tol): "
           "steps applied, as a backward-stable direct solver's would be";
    return s;
  }
};

}  // namespace sgo
