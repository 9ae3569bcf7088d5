// clu_plan.h -- how a round call (fclu_round_exact, fclu_round_bnb, fclu_round_bnb_wide in freddie_cluster.hip) cuts the problems it takes
// into workgroup items and launches.  Plain host code without a HIP call: tools/plan_host_check.cpp runs it under the address and
// undefined-behaviour sanitizers where there is no GPU.
//
// A problem has a number of units (the exact solve: its 2^R masks; the searches: its 2^min(R, depth) tasks) and a unit costs unit_cost of
// the call's budget (1; node_cap).  Problems are taken in the order given -- ascending (columns, problem) -- while the budget holds; the
// first that does not fit ends the taking, since nothing behind it is smaller.  A taken problem's units are cut into items of at most
// wg_units, an item never crosses a launch, and a launch holds at most launch_units units and asks for the largest LDS size among its items.
#ifndef CLU_PLAN_H
#define CLU_PLAN_H

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

struct PlanItem { int prob, first, n, pad; };      // a workgroup's work: problem, first unit, units (the kernels read it as an int4)

struct LaunchPlan {
    std::vector<int> list;                         // the taken problems, in the order they were taken
    std::vector<PlanItem> items;
    std::vector<size_t> launch_first;              // a launch's first item; closed by the number of items
    std::vector<size_t> launch_lds;                // a launch's dynamic LDS bytes
    std::vector<long long> unit_off, n_units;      // per problem of the round: its first unit among the taken ones' and its units (0, 0: not taken)
    long long total_units = 0;
    size_t n_launch() const { return launch_lds.size(); }
};

// order: (columns, problem) of the candidates, sorted; units_of(problem) >= 1 and lds_of(problem) are the caller's; unit_cost, wg_units and
// launch_units are at least 1.
template <typename Units, typename Lds>
LaunchPlan plan_launches(const std::vector<std::pair<int, int>> &order, size_t n_prob, Units units_of, long long unit_cost, long long budget, long long wg_units,
                         long long launch_units, Lds lds_of) {
    LaunchPlan pl;
    pl.unit_off.assign(n_prob, 0);
    pl.n_units.assign(n_prob, 0);
    long long spent = 0, in_launch = 0;
    for (const auto &rp : order) {
        const int p = rp.second;
        const long long units = units_of(p);
        // no product that could overflow; with a unit cost of 1 this is "total so far + units > budget"
        if (units > (budget - spent) / unit_cost) break;
        spent += units * unit_cost;
        pl.list.push_back(p);
        pl.unit_off[(size_t)p] = pl.total_units; pl.n_units[(size_t)p] = units;
        pl.total_units += units;
        const size_t lds = lds_of(p);
        for (long long lo = 0; lo < units; lo += wg_units) {
            const long long n = std::min(wg_units, units - lo);
            if (pl.launch_lds.empty() || in_launch + n > launch_units) { pl.launch_first.push_back(pl.items.size()); pl.launch_lds.push_back(0); in_launch = 0; }
            pl.items.push_back(PlanItem{p, (int)lo, (int)n, 0});
            pl.launch_lds.back() = std::max(pl.launch_lds.back(), lds);
            in_launch += n;
        }
    }
    pl.launch_first.push_back(pl.items.size());
    return pl;
}

#endif
