// plan_host_check.cpp -- the launch planner of the round calls (freddie_amd/csrc/clu_plan.h, what fclu_round_exact, fclu_round_bnb and
// fclu_round_bnb_wide of freddie_cluster.hip cut their problems into items and launches with) on hand-built orders, as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_plan_host.py builds and runs it; no GPU).  Every check that
// fails prints its line; the exit status is the number of failures, and the last line of output the number of checks.
#include "clu_plan.h"

#include <climits>
#include <cstdio>

typedef long long i64;
typedef std::vector<std::pair<int, int>> Order;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond) \
    do { ++n_checks; if (!(cond)) { ++n_failed; printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// a plan over problems whose units and LDS sizes are given per problem; the order's first member is the unit count (any ascending key does)
static LaunchPlan plan(const std::vector<i64> &units, i64 unit_cost, i64 budget, i64 wg_units, i64 launch_units, const std::vector<size_t> &lds = {}) {
    Order order;
    for (size_t p = 0; p < units.size(); ++p) order.emplace_back((int)std::min<i64>(units[p], INT_MAX), (int)p);
    std::sort(order.begin(), order.end());
    return plan_launches(order, units.size(), [&](int p) { return units[(size_t)p]; }, unit_cost, budget, wg_units, launch_units,
                         [&](int p) { return lds.empty() ? (size_t)16 : lds[(size_t)p]; });
}

// what holds of every plan: the items cover each taken problem's units once and in order, no item is larger than a workgroup, no launch
// than launch_units, the launches partition the items, the offsets run through the taken problems
static void check_shape(const LaunchPlan &pl, const std::vector<i64> &units, i64 wg_units, i64 launch_units) {
    CHECK(pl.launch_first.size() == pl.n_launch() + 1 && pl.launch_first.back() == pl.items.size());
    CHECK(pl.unit_off.size() == units.size() && pl.n_units.size() == units.size());
    size_t at = 0;
    i64 off = 0;
    for (const int p : pl.list) {
        CHECK(pl.unit_off[(size_t)p] == off && pl.n_units[(size_t)p] == units[(size_t)p]);
        for (i64 lo = 0; lo < units[(size_t)p]; ++at) {
            CHECK(at < pl.items.size());
            if (at >= pl.items.size()) return;
            const PlanItem &it = pl.items[at];
            CHECK(it.prob == p && it.first == lo && it.n >= 1 && it.n <= wg_units && it.pad == 0);
            lo += it.n;
        }
        off += units[(size_t)p];
    }
    CHECK(at == pl.items.size() && off == pl.total_units);
    for (size_t l = 0; l < pl.n_launch(); ++l) {
        i64 in_launch = 0;
        CHECK(pl.launch_first[l] < pl.launch_first[l + 1]);
        for (size_t i = pl.launch_first[l]; i < pl.launch_first[l + 1]; ++i) in_launch += pl.items[i].n;
        CHECK(in_launch <= launch_units);
    }
}

int main() {
    {   // an empty order: nothing taken, no launch, the closing entry alone
        const LaunchPlan pl = plan({}, 1, 1000, 64, 1024);
        CHECK(pl.list.empty() && pl.items.empty() && pl.n_launch() == 0 && pl.total_units == 0 && pl.launch_first == std::vector<size_t>{0});
    }
    {   // one problem smaller than a workgroup
        const LaunchPlan pl = plan({8}, 4096, 1ll << 40, 256, 4096, {48});
        check_shape(pl, {8}, 256, 4096);
        CHECK(pl.items.size() == 1 && pl.items[0].n == 8 && pl.n_launch() == 1 && pl.launch_lds[0] == 48);
    }
    {   // one problem across several launches (a 12-column problem with 64 masks a workgroup and 1024 a launch) and a small one in front
        const LaunchPlan pl = plan({4096, 8}, 1, 1ll << 40, 64, 1024);
        check_shape(pl, {4096, 8}, 64, 1024);
        CHECK(pl.list == std::vector<int>({1, 0}) && pl.items.size() == 65 && pl.total_units == 4096 + 8);
        CHECK(pl.n_launch() == 5 && pl.launch_first == std::vector<size_t>({0, 16, 32, 48, 64, 65}));
    }
    {   // the counts the GPU tests assert: one task a launch (8 + 32 + 32), 40 a launch, and the wide call's 1 and 11 with 8 a workgroup
        CHECK(plan({8, 32, 32}, 4096, 1ll << 40, 1, 1).n_launch() == 8 + 32 + 32);
        const LaunchPlan some = plan({8, 32, 32}, 4096, 1ll << 40, 40, 40);
        check_shape(some, {8, 32, 32}, 40, 40);
        CHECK(some.n_launch() == 2 && some.items.size() == 3);
        CHECK(plan({16, 16, 16}, 4096, 1ll << 40, 1, 1).n_launch() == 3 * 16);
        const LaunchPlan wide = plan({16, 16, 16}, 4096, 1ll << 40, 8, 11);
        check_shape(wide, {16, 16, 16}, 8, 11);
        CHECK(wide.n_launch() == 6 && wide.items.size() == 6);
        CHECK(plan({1 << 13, 1 << 13, 1 << 13}, 1, 1ll << 40, 1, 1).n_launch() == 3 * (1 << 13));      // (more than the 4096 a call issues)
    }
    {   // a launch asks for the largest LDS size among its items
        const LaunchPlan pl = plan({4, 12}, 1, 1000, 4, 8, {100, 300});
        check_shape(pl, {4, 12}, 4, 8);
        CHECK(pl.n_launch() == 2 && pl.launch_lds == std::vector<size_t>({300, 300}));
        const LaunchPlan alone = plan({8, 12}, 1, 1000, 4, 8, {100, 300});
        CHECK(alone.n_launch() == 3 && alone.launch_lds == std::vector<size_t>({100, 300, 300}));
    }
    {   // the budget ends the taking on the first, a middle and no problem: 16 tasks of 10 nodes each, 160 a problem
        const std::vector<i64> units = {16, 16, 16};
        const struct { i64 budget; size_t taken; } cases[] = {{1, 0}, {159, 0}, {160, 1}, {319, 1}, {320, 2}, {479, 2}, {480, 3}, {1ll << 40, 3}};
        for (const auto &cs : cases) {
            const LaunchPlan pl = plan(units, 10, cs.budget, 8, 1 << 20);
            check_shape(pl, units, 8, 1 << 20);
            CHECK(pl.list.size() == cs.taken && pl.total_units == 16 * (i64)cs.taken);
            for (size_t p = cs.taken; p < units.size(); ++p) CHECK(pl.unit_off[p] == 0 && pl.n_units[p] == 0);
        }
    }
    {   // a unit cost of 1 against "total so far + units > budget", the exact call's test as it was written before
        const std::vector<i64> units = {2, 8, 8, 64, 4096};
        for (i64 budget = 1; budget <= 4200; ++budget) {
            size_t taken = 0;
            i64 total = 0;
            while (taken < units.size() && !(total + units[taken] > budget)) total += units[taken++];
            const LaunchPlan pl = plan(units, 1, budget, 64, 1024);
            CHECK(pl.list.size() == taken && pl.total_units == total);
        }
    }
    {   // budgets and unit costs near 2^62: no product is formed that the budget does not hold
        const i64 big = 1ll << 62;
        CHECK(plan({1, 1}, (1ll << 61) + 1, big, 1, 1).list.size() == 1);
        CHECK(plan({2, 2}, 1ll << 61, big, 1, 1).list.size() == 1);
        CHECK(plan({1 << 20}, 1ll << 61, big, 256, 4096).list.empty());
        CHECK(plan({3}, big, big, 1, 1).list.empty());
        CHECK(plan({1, 1}, big, big, 1, 1).list.size() == 1);
        const LaunchPlan pl = plan({1 << 24, 1 << 24}, 1, LLONG_MAX, 4096, 1 << 24);
        CHECK(pl.list.size() == 2 && pl.n_launch() == 2 && pl.items.size() == 2 * 4096);
    }
    printf("%d checks, %d failed\n", n_checks, n_failed);
    return n_failed ? 1 : 0;
}
