"""The clustering stage from segment_*.tsv to cluster_*.tsv: the reference's cluster_tint() (py/freddie_cluster.py:694-780) restated
with its loop turned inside out.  The reference runs the rounds of one partition after the other; rounds of different partitions do
not depend on each other, so here round r of EVERY active partition of every tint of a batch is one device call
(cluster_prep.Context.round_models: informative segments, support, correction terms, pairs, gap groups) followed by the solves
(cluster_solve.solve_round: HiGHS; a process pool when asked for), and the results are put back in the reference's order.

  cluster_tint :716-773   -> cluster_tints()        min_isoform_size, max_rounds, the breaks and garbage_rids as there
  run_ilp's read-out :601-635 -> read_out()         isoform exons = e on informative segments, the first remaining rep's I elsewhere;
                                                     corrections = the rep's first read's data, '-' where uninformative, 'X' where C, x and e
  output_isoforms :639-691 -> output_isoforms()
The solve is HiGHS, not Gurobi: where a round's optimum is not unique the tie may be broken differently.  Under
settings["incumbent"] = "cutoff" / "fallback" a round is one more device call (Context.round_incumbents: a greedy feasible isoform per
problem), which bounds the solves and, under "fallback", answers for a solve that ends without a proven optimum.  Under
settings["exact_cols"] = N > 0 a round is one more device call (Context.round_exact): every problem of at most N columns that fits the
mask budget is solved there by enumeration, a proven optimum, and only the others go to the solver.  Under settings["bnb_cols"] = N >
exact_cols the problems of exact_cols + 1 .. N (<= 64) columns that fit the node budget are searched by a branch and bound on the device
(Context.round_bnb, behind a round_incumbents call whose costs bound it): a search that finishes is a proven optimum under the
enumeration's rule and makes no solve job; one that does not hands the solver its best set as an incumbent.  Under
settings["device_rounds"] (with exact_cols, bnb_cols or wide_cols) the models of a round stay on the device (round_models(fetch=False)); the problems
the GPU has answered get their isoforms from one more device call (Context.round_readout) and no model, list or loop of theirs is built
on the host, and only the other problems are modelled again, alone, for the solver.  Under settings["wide_cols"] = N > max(exact_cols,
bnb_cols) the problems of more columns than those and at most N (<= 1024) whose tables fit are searched by the same branch and bound on
sets of several words (Context.round_bnb_wide), and answered exactly as round_bnb's are."""
import os

import numpy as np

from . import cluster_prep, cluster_solve

MAX_WORKERS = 16
FILES_PER_BATCH = 256


EXACT_MASKS = 1 << 29     # the default mask budget of a round's exact call: what keeps the call at 24 columns under a round_models call on the
                          # cluster-many workload (profiles/cluster_exact.txt)


BNB_NODES = 1 << 30       # the default node budget of a round's branch and bound: 16 384 problems at BNB_DEPTH and BNB_NODE_CAP (2^6 tasks x 1024
                          # nodes each), 64 launches -- ten times the 1 672 problems of 25 to 64 columns of the cluster-many workload's first round
                          # (profiles/cluster_bnb.txt)


WIDE_MAX_PASSES = 16      # passes of a round's wide branch and bound at the most (cluster_prep.BNB_WIDE_MAX_PASSES, the library's limit)
WIDE_NODES = 1 << 30      # the default node budget of a round's wide branch and bound: the sum of tasks x node cap over the problems it takes
                          # (profiles/cluster_bnb_wide.txt)


def ilp_settings(recycle_model="constant", epsilon=0.2, offset=20, timeout=1, max_rounds=30, min_isoform_size=3, max_ilp=1000, incumbent="off",
                 exact_cols=0, exact_masks=EXACT_MASKS, bnb_cols=0, bnb_nodes=BNB_NODES, device_rounds=False, wide_cols=0, wide_nodes=WIDE_NODES,
                 wide_passes=1):
    """incumbent: "off"; "cutoff": every round's greedy incumbents (Context.round_incumbents, one device call a round) bound the solves'
    objective; "fallback": and stand in for a solve that ends without a proven optimum (status INCUMBENT).
    exact_cols: 0, or the largest number of columns (<= 24) of a problem the GPU solves exactly by enumeration (Context.round_exact, one
    device call a round) instead of the solver; exact_masks: that call's budget, the sum of 2^columns over the problems it takes.
    bnb_cols: 0, or the largest number of columns (<= 64) of a problem the GPU searches by branch and bound (Context.round_bnb: the problems
    of exact_cols + 1 .. bnb_cols columns; one more device call a round, two where the incumbents are not computed anyway); bnb_nodes: that
    call's budget, the sum of tasks x node cap over the problems it takes.
    device_rounds: the round's models stay on the device and the problems the GPU has answered are read out there (Context.round_readout);
    it needs exact_cols, bnb_cols or wide_cols, the calls that answer problems.
    wide_cols: 0, or the largest number of columns (<= 1024) of a problem the GPU searches by the branch and bound on sets of several words
    (Context.round_bnb_wide: the problems of max(exact_cols, bnb_cols) + 1 .. wide_cols columns whose tables fit); wide_nodes: that call's
    budget, as bnb_nodes, a pass; wide_passes: 1 .. 16, the passes of that call (cluster_solve.exact_bnb_wide(passes=...)): beyond the
    first, the open subtrees of the tasks that stopped at the node cap are searched as tasks of their own.  1: the single search."""
    if device_rounds and not (exact_cols > 0 or bnb_cols > 0 or wide_cols > 0):
        raise ValueError("device_rounds needs exact_cols, bnb_cols or wide_cols: without them no problem is answered on the device")
    return dict(recycle_model=recycle_model, K=2, epsilon=epsilon, offset=offset, timeout=timeout, max_rounds=max_rounds, threads=1,
                min_isoform_size=min_isoform_size, max_ilp=max_ilp, incumbent=incumbent, exact_cols=exact_cols, exact_masks=exact_masks,
                bnb_cols=bnb_cols, bnb_nodes=bnb_nodes, device_rounds=bool(device_rounds), wide_cols=wide_cols, wide_nodes=wide_nodes,
                wide_passes=wide_passes)


def check_exact(settings):
    cols, masks = settings.get("exact_cols", 0), settings.get("exact_masks", EXACT_MASKS)
    if not 0 <= cols <= cluster_solve.EXACT_MAX_COLS:
        raise ValueError("exact_cols is %r: 0 .. %d" % (cols, cluster_solve.EXACT_MAX_COLS))
    if cols and masks < 1:
        raise ValueError("exact_masks is %r: at least 1" % (masks,))


def check_bnb(settings):
    cols, nodes = settings.get("bnb_cols", 0), settings.get("bnb_nodes", BNB_NODES)
    if not 0 <= cols <= cluster_solve.BNB_MAX_COLS:
        raise ValueError("bnb_cols is %r: 0 .. %d" % (cols, cluster_solve.BNB_MAX_COLS))
    if cols and nodes < 1:
        raise ValueError("bnb_nodes is %r: at least 1" % (nodes,))


def check_wide(settings):
    cols, nodes = settings.get("wide_cols", 0), settings.get("wide_nodes", WIDE_NODES)
    if not 0 <= cols <= cluster_solve.BNB_WIDE_MAX_COLS:
        raise ValueError("wide_cols is %r: 0 .. %d" % (cols, cluster_solve.BNB_WIDE_MAX_COLS))
    if cols and nodes < 1:
        raise ValueError("wide_nodes is %r: at least 1" % (nodes,))
    passes = settings.get("wide_passes", 1)
    if not (isinstance(passes, int) and 1 <= passes <= WIDE_MAX_PASSES):
        raise ValueError("wide_passes is %r: 1 .. %d" % (passes, WIDE_MAX_PASSES))


def check_device_rounds(settings):
    if settings.get("device_rounds", False) and not (settings.get("exact_cols", 0) > 0 or settings.get("bnb_cols", 0) > 0 or settings.get("wide_cols", 0) > 0):
        raise ValueError("device_rounds needs exact_cols, bnb_cols or wide_cols: without them no problem is answered on the device")


def garbage_costs(tint, recycle_model):
    """Per rep, the three garbage costs as the reference's formulas read (:186-194, :314-322); its own preprocess_ilp() hands the
    exons / introns formulas a list where they want a dict and raises, so only their evident meaning can be restated."""
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    out = {}
    for i, members in enumerate(tint["read_reps"]):
        if recycle_model == "exons":
            out[i] = len(members) * max(sum(I[i]) - 0.5, 1)
        elif recycle_model == "introns":
            out[i] = len(members) * max(sum(C[i]) - 0.5, 1)
        else:
            out[i] = len(members) * 3
    return out


def read_out(tint, remaining, model, x, e):
    """The round's isoform as run_ilp() returns it (:601-635): dict(exons, rid_to_corrections)."""
    M = len(tint["segs"])
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    e_of = dict(zip(model["inf_seg"], e))
    exons = [e_of[j] if j in e_of else I[remaining[0]][j] for j in range(M)]
    rid_to_corrections = dict()
    for c, i in enumerate(remaining):
        if not x[c]:
            continue
        data = tint["reads"][tint["read_reps"][i][0]]["data"]
        corrections = [str(data[j]) for j in range(M)]
        for j in range(M):
            if j not in e_of:
                corrections[j] = "-"
            elif C[i][j] == 1 and e_of[j]:
                corrections[j] = "X"
        rid_to_corrections[i] = corrections
    return dict(exons=exons, rid_to_corrections=rid_to_corrections)


def _read_line(read, isoform, labels):
    out = [str(read["id"]), read["name"], read["chr"], read["strand"], str(read["tint"]), str(read["partition"]),
           str(read["poly_tail_category"]), isoform, "".join(map(str, labels))]
    exon_strs = [str(v) for v in labels]
    for (j1, _), l in read["gaps"].items():
        exon_strs[j1] += "({})".format(l)                    # (j1 = -1, a start tail's pseudo-gap, lands on the last segment, as there)
    out.extend(exon_strs)
    out.extend("{}:{}".format(k, v) for k, v in sorted(read["poly_tail"].items()))
    return "\t".join(out) + "\n"


def output_isoforms(tint, out_file):
    """cluster_*.tsv of one tint (:639-691)."""
    reads, read_reps = tint["reads"], tint["read_reps"]
    out_file.write("#{}\t{}\t{}\n".format(tint["chr"], tint["id"], ",".join([str(s[0]) for s in tint["segs"]] + [str(tint["segs"][-1][1])])))
    for iid, isoform in enumerate(tint["isoforms"]):
        out_file.write("isoform_{}\t{}\t{}\n".format(iid, tint["id"], "".join(map(str, isoform["exons"]))))
        for i, corrections in isoform["rid_to_corrections"].items():
            for ridx in read_reps[i]:
                out_file.write(_read_line(reads[ridx], str(iid), corrections))
    for i in tint["garbage_rids"]:
        for ridx in read_reps[i]:
            out_file.write(_read_line(reads[ridx], "*", reads[ridx]["data"]))


def _solve_job(job):
    solve, model, settings = job
    return solve(model, settings)


def _refused_error(tint, s, round_num, column):
    return cluster_prep.ClusterError("tint %s partition %d round %d: a gap of column %d (rep %d) ends on an uninformative segment "
                                     "(the reference's assert, py/freddie_cluster.py:467-468)" % (tint["id"], s["q"], round_num, column, s["remaining"][column]))


def _gpu_answer(exact, bnb, greedy, p, wide=None):
    """(found, incumbent) of problem p from the round's exact and branch-and-bound calls: found = (cost, x), "infeasible" or None (the
    solver's); incumbent = what an unproven search hands the solver, the better of its best set and the greedy's, or None."""
    found = cluster_prep.round_exact_solution(exact, p) if exact is not None else None
    incumbent = None
    if found is None and bnb is not None:
        found = cluster_prep.round_bnb_solution(bnb, p)
    if found is None and wide is not None:                   # (a problem is taken by one search at the most: the sizes do not overlap)
        found = cluster_prep.round_bnb_wide_solution(wide, p)
    if found is not None and found[0] == "unproven":
        if found[1] is not None:
            best = cluster_prep.round_incumbent(greedy, p)
            incumbent = tuple(found[1:]) if best is None or found[1] < best[0] else best
        found = None
    return found, incumbent


def _members_e(tint, remaining, members, arr, p):
    """e of a column set as the model defines it -- the OR of the members' I bits on problem p's informative segments -- on the host, for
    a proven problem that got no set in the read-out (too small for an isoform, or empty) and a caller that still wants its e."""
    words = arr["inf_bits"][int(arr["inf_bits_off"][p]):int(arr["inf_bits_off"][p + 1])]
    I = tint["ilp_data"]["I"]
    rows = [I[remaining[c]] for c in members]
    return [int(any(row[j] for row in rows)) for j in range(len(tint["segs"])) if (int(words[j >> 5]) >> (j & 31)) & 1]


def _device_round(ctx, tints, todo, parts, arr, found, min_size, round_num):
    """A round under device_rounds behind the resident round_models() call and the solves: which problems the device has answered
    (direct: p -> (status, x, cost, the isoform's size, members)), the one round_readout() call for those that are isoforms (out; a
    problem below min_size gets no set), and the other problems (host) modelled by a second, fetched call on them alone (sub; none left:
    no call).  A refused problem raises as it does without the flag."""
    for p, s in enumerate(todo):
        if arr["refused"][p] >= 0:
            raise _refused_error(tints[s["t"]], s, round_num, int(arr["refused"][p]))
    direct, host, sets = {}, [], [[] for _ in todo]
    for p, s in enumerate(todo):
        answer = found[p][0]
        if answer == "infeasible":
            direct[p] = (cluster_solve.NO_SOLUTION, None, None, 0, [])
        elif answer is not None and (min_size > 0 or any(answer[1])):       # (an empty isoform that counts, min_size 0, takes the host's way)
            members = [c for c, v in enumerate(answer[1]) if v]
            size = int(tints[s["t"]]["rep_weight"][np.asarray(s["remaining"], np.int64)[members]].sum()) if members else 0
            if members and size >= min_size:
                sets[p] = members
            direct[p] = (cluster_solve.OPTIMAL, answer[1], answer[0], size, members)
        else:
            host.append(p)
    out = ctx.round_readout(sets) if any(sets) else None
    sub = ctx.round_models([parts[p] for p in host], [todo[p]["remaining"] for p in host]) if host else None
    return direct, host, out, sub


def cluster_tints(tints, part0, ctx, settings, solve=cluster_solve.solve_round, pool=None, on_round=None, round_model=None):
    """The rounds of every partition of preprocessed, partitioned tints whose rows the context holds (Context.partition_segment() /
    partition_labels() and round_setup()); part0[t] = the batch's number of tint t's first partition.  Leaves tint['isoforms'],
    tint['garbage_rids'] and the reads' 'partition' as cluster_tint() does, and returns per tint the timeout.log lines
    [(status, tint id, partition, round, remaining reps)].  on_round: called with a dict per solved round (tests, profiles).
    round_model: what cuts problem p out of a round_models() result, cluster_prep.round_model by default (a caller's wrapper counts)."""
    cluster_solve.check_settings(settings)
    check_exact(settings)
    check_bnb(settings)
    check_wide(settings)
    check_device_rounds(settings)
    device = bool(settings.get("device_rounds", False))
    build_model = round_model if round_model is not None else (lambda arr, p: cluster_prep.round_model(arr, p))
    min_size, max_rounds = settings["min_isoform_size"], settings["max_rounds"]
    state = []                                               # a partition: its tint, number, remaining reps, isoforms; active or not
    for t, tint in enumerate(tints):
        tint["garbage_cost"] = garbage_costs(tint, settings["recycle_model"])
        tint["max_lg"] = sum(s[2] for s in tint["segs"])
        if device:
            tint["rep_weight"] = np.array([len(members) for members in tint["read_reps"]], np.int64)
        for q, (rids, incomp) in enumerate(tint["partitions"]):
            for rid in rids:
                for ridx in tint["read_reps"][rid]:
                    tint["reads"][ridx]["partition"] = q
            state.append(dict(t=t, q=q, remaining=list(rids), incomp=incomp, isoforms=[], active=True))
    logs = [[] for _ in tints]
    for round_num in range(max_rounds):
        todo = []
        for s in state:
            if s["active"] and sum(len(tints[s["t"]]["read_reps"][i]) for i in s["remaining"]) < min_size:
                s["active"] = False                          # (:729-730)
            if s["active"]:
                todo.append(s)
        if not todo:
            break
        parts = [part0[s["t"]] + s["q"] for s in todo]
        arr = ctx.round_models(parts, [s["remaining"] for s in todo], fetch=False) if device else ctx.round_models(parts, [s["remaining"] for s in todo])
        inc = None
        if settings.get("incumbent", "off") != "off":        # one more device call behind the models; a refused problem raises below
            inc = ctx.round_incumbents([g for s in todo for g in (tints[s["t"]]["garbage_cost"][i] for i in s["remaining"])],
                                       settings["epsilon"], settings["offset"])
        exact = None
        if settings.get("exact_cols", 0) > 0:                # one more device call: the small problems' proven optima, no solve job for them
            exact = ctx.round_exact([g for s in todo for g in (tints[s["t"]]["garbage_cost"][i] for i in s["remaining"])],
                                    settings["epsilon"], settings["offset"], settings["exact_cols"], settings.get("exact_masks", EXACT_MASKS))
        bnb = greedy = None
        if settings.get("bnb_cols", 0) > settings.get("exact_cols", 0):     # the larger problems' search, bounded by the greedy incumbents' costs
            garbage = [g for s in todo for g in (tints[s["t"]]["garbage_cost"][i] for i in s["remaining"])]
            greedy = inc if inc is not None else ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])
            bnb = ctx.round_bnb(garbage, greedy["cost2"], settings["epsilon"], settings["offset"], settings.get("exact_cols", 0) + 1, settings["bnb_cols"],
                                settings.get("bnb_nodes", BNB_NODES))
        wide = None
        narrow_cols = max(settings.get("exact_cols", 0), settings.get("bnb_cols", 0))
        if settings.get("wide_cols", 0) > narrow_cols:       # the same search on sets of several words, for the problems beyond both
            garbage = [g for s in todo for g in (tints[s["t"]]["garbage_cost"][i] for i in s["remaining"])]
            if greedy is None:
                greedy = inc if inc is not None else ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])
            passes = settings.get("wide_passes", 1)          # (1: the call of before, without the argument)
            wide =ctx.round_bnb_wide(garbage, greedy["cost2"], settings["epsilon"], settings["offset"], narrow_cols + 1, settings["wide_cols"],
                                      settings.get("wide_nodes", WIDE_NODES), **({"passes": passes} if passes > 1 else {}))
        # ---- every problem's answer from the device, once; under device rounds the answered ones get no model
        found = [_gpu_answer(exact, bnb, greedy, p, wide) for p in range(len(todo))]
        direct, host, out, source = {}, list(range(len(todo))), None, arr
        if device:
            direct, host, out, source = _device_round(ctx, tints, todo, parts, arr, found, min_size, round_num)
        jobs, models, answers = [], {}, {}
        for k, p in enumerate(host):
            s = todo[p]
            tint = tints[s["t"]]
            slot = k if device else p                        # (the second call holds the host's problems alone)
            model = build_model(source, slot)
            if model is None:
                raise _refused_error(tint, s, round_num, int(source["refused"][slot]))
            model["garbage"] = [tint["garbage_cost"][i] for i in s["remaining"]]
            model["max_lg"] = tint["max_lg"]
            model["key"] = (tint["id"], s["q"], round_num)        # (for a solver that logs, or replays: tests)
            if inc is not None:
                model["incumbent"] = cluster_prep.round_incumbent(inc, p)
            models[p] = model
            answer, incumbent = found[p]                     # (unproven: the solver's, with the better of the search's set and the greedy's
            if incumbent is not None:                        # as its incumbent)
                model["incumbent"] = incumbent
            if answer is None:
                answers[p] = len(jobs)                       # the solver's: its place among the jobs
                jobs.append((solve, model, settings))
            elif answer == "infeasible":
                answers[p] = (cluster_solve.NO_SOLUTION, None, None)
            else:
                x = answer[1]
                answers[p] = (cluster_solve.OPTIMAL, x, [int(any(x[c] for c in support)) for support in model["support"]])
        results = pool.map(_solve_job, jobs, chunksize=1) if pool is not None else [_solve_job(j) for j in jobs]
        for p, s in enumerate(todo):
            tint = tints[s["t"]]
            if p in direct:                                  # answered on the device; read out there where it is an isoform
                status, x, cost, size, members = direct[p]
                got = cluster_prep.readout_isoform(out, p, s["remaining"]) if out is not None else None
                isoform, e = got if got is not None else (None, None)
                if isoform is None and status == cluster_solve.OPTIMAL and on_round is not None:
                    e = _members_e(tint, s["remaining"], members, arr, p)      # (no set, so no e from the call: the callback's alone)
            else:
                model, answer = models[p], answers[p]
                status, x, e = results[answer] if isinstance(answer, int) else answer
                cost = cluster_solve.round_cost(model, x, e) if status in (cluster_solve.OPTIMAL, cluster_solve.INCUMBENT) else None
            logs[s["t"]].append((status, tint["id"], s["q"], round_num, len(s["remaining"])))
            if on_round is not None:
                on_round(dict(tint=tint, partition=s["q"], round=round_num, remaining=list(s["remaining"]), incomp=s["incomp"], status=status,
                              cost=cost, x=x, e=e))
            if status not in (cluster_solve.OPTIMAL, cluster_solve.INCUMBENT):
                s["active"] = False                          # (:750-751)
                continue
            if p not in direct:
                isoform = read_out(tint, s["remaining"], model, x, e)
                size = sum(len(tint["read_reps"][rid]) for rid in isoform["rid_to_corrections"])
            if size < min_size:
                s["active"] = False                          # (:755-756; with one isoform a round, :758-759 is the same test)
                continue
            s["isoforms"].append(isoform)
            for rid in isoform["rid_to_corrections"]:
                s["remaining"].remove(rid)
    for t, tint in enumerate(tints):
        tint["isoforms"], tint["garbage_rids"] = [], []
    for s in state:                                          # the reference's order: partition by partition, a partition's rounds in order
        tint = tints[s["t"]]
        for isoform in s["isoforms"]:
            tint["isoforms"].append(isoform)
            for rid, corrections in isoform["rid_to_corrections"].items():
                for ridx in tint["read_reps"][rid]:
                    tint["reads"][ridx]["corrections"] = corrections
                    tint["reads"][ridx]["isoform"] = len(tint["isoforms"]) - 1
        tint["garbage_rids"].extend(sorted(s["remaining"]))
    return [sorted(lines, key=lambda l: (l[2], l[3])) for lines in logs]


def stage_files(paths, settings, ctx, threads=8):
    """segment_*.tsv files -> (tints as preprocess_ilp() + partition_reads() leave them, part0), rows and pair lists on the context."""
    arrays = cluster_prep.read_segment_arrays(paths, threads)
    groups, prep, arr = ctx.partition_segment(arrays, settings["max_ilp"])
    tints = cluster_prep.tints_from_arrays(arrays, groups, prep, arr, dict(recycle_model="constant"))
    ctx.round_setup(*cluster_prep.round_gaps(tints))
    return tints, arr["tint_part_off"].tolist(), arrays.file_tint_off.tolist()


def cluster_files(paths, settings, ctx, solve=cluster_solve.solve_round, pool=None, on_round=None, threads=8, round_model=None):
    """Yields (tints of the file, their timeout.log lines) per path, in order, a batch of FILES_PER_BATCH files at a time as it finishes
    (a caller that writes as it goes keeps one batch in memory and loses nothing finished to a late failure); a batch whose pair list
    the library refuses as too large for one call is halved."""
    for b0 in range(0, len(paths), FILES_PER_BATCH):
        pending = [list(paths[b0:b0 + FILES_PER_BATCH])]
        while pending:
            batch = pending.pop(0)
            try:
                tints, part0, file_off = stage_files(batch, settings, ctx, threads)
            except cluster_prep.ClusterError as err:
                if err.code != cluster_prep.ERR_UNSUPPORTED or len(batch) < 2:
                    raise
                pending[:0] = [batch[:len(batch) // 2], batch[len(batch) // 2:]]
                continue
            logs = cluster_tints(tints, part0, ctx, settings, solve, pool, on_round, round_model)
            for f in range(len(batch)):
                yield tints[file_off[f]:file_off[f + 1]], logs[file_off[f]:file_off[f + 1]]


EXACT_HELP = ("Recommended where small problems dominate: 24 -- measured on an MI355X (profiles/cluster_exact.txt), the enumeration beats HiGHS at every "
              "size up to 24 columns; the budget, not N, bounds a call.")


BNB_HELP = ("Recommended: 64 -- measured on an MI355X (profiles/cluster_bnb.txt), a call proves 1 652 of the cluster-many workload's 1 672 problems of 25 "
            "to 64 columns in 0.28 s, where sixteen HiGHS workers take about 21 s.")


WIDE_HELP = ("Recommended: 128 -- measured on an MI355X (profiles/cluster_bnb_wide.txt; the first round of the first 40 files of the cluster-many "
             "workload, written without gaps), a call proves all 160 problems of 120 to 124 columns under -mi 128 in 12 ms, where sixteen HiGHS "
             "workers take 5.2 s for 16 of them.  Not recommended above 128: under -mi 256 a call proves 4 of 80 problems of about 245 columns "
             "within 50 ms a launch (64 of 80 with 16 384 nodes a task, 69 ms a launch), and under -mi 1000 none of 40 problems of about 490 "
             "columns; the best sets found still reach the solver as incumbents.  A task's node cap follows the largest problem of a round "
             "that N admits (4 096 up to 128 columns, 8 192 up to 256, 4 096 beyond), so a larger N changes the cap of the smaller problems too.")


WIDE_PASSES_HELP = ("Measured per call on an MI355X (profiles/cluster_bnb_wide_passes.txt): under -mi 256, 4 096 nodes a task and 8 passes prove 80 of 80 "
                    "problems of about 245 columns in 89 ms with no launch over 18 ms, where the single pass proves 4 of 80; under -mi 1000 nothing is "
                    "proven with 8 passes either.  The whole loop with the flag has not been measured, so the default stays 1.")


DEVICE_ROUNDS_HELP = ("Recommended together with --exact-small 24 --exact-bnb 64 at small maximum ILP sizes: measured on an MI355X "
                      "(profiles/cluster_device_rounds.txt; the first 40 of the cluster-many workload's 400 files, written without gaps, sixteen "
                      "workers, medians of three runs) the whole loop takes 10.3 s against 26.7 s under -mi 24 and 2.8 s against 18.1 s under "
                      "-mi 64, far more than the runs differ (1.8 s, 3.9 s), with the same output.  Not recommended under -mi 1000: on the same "
                      "40 files the loop is the solver's (one round, 40 solves) and takes 195.4 s and 198.0 s with the flag "
                      "against 197.0 s to 198.8 s without, no more than the runs differ.")


# ---- the command line (py/freddie_cluster.py :37-110, :783-827) ---------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(
        description="Cluster aligned reads into isoforms.  The rounds' models are built on the GPU; the solve is HiGHS (scipy.optimize.milp), "
                    "not Gurobi: optimal ties may be broken differently from Gurobi's.  The .lp, .glog and .sol files are Gurobi's and are not "
                    "written; --logs-dir holds the timeout.log files, with this program's status (OPTIMAL / NO_SOLUTION, INCUMBENT under "
                    "--incumbent fallback) in the first column.")
    recycle_models = ["constant", "exons", "introns", "relative"]
    parser.add_argument("-s", "--segment-dir", type=str, required=True, help="Path to Freddie segment directory of the reads")
    parser.add_argument("-rm", "--recycle-model", type=str, default="constant",
                        help="Model type: {}. Default: {}.  relative is refused: it needs E2I_min".format(", ".join(recycle_models), "constant"))
    parser.add_argument("-go", "--gap-offset", type=int, default=20, help="Slack +- value for exons and the unaligned gaps. Default: 20")
    parser.add_argument("-e", "--epsilon", type=float, default=0.2, help="Epsilon percent value for how much can unaligned gaps can cover. Default: 0.2")
    parser.add_argument("-mr", "--max-rounds", type=int, default=30, help="Maximum number of ILP rounds. Default 30")
    parser.add_argument("-is", "--min-isoform-size", type=int, default=3, help="Minimum isoform size in terms of number supporting reads. Default 3")
    parser.add_argument("-mi", "--max-ilp", type=int, default=1000,
                        help="Maximum number of unique reads allowed for an ILP instance. ILP instances with more reads will have their input "
                             "broken into evenly sized problems, each with less than the max. Default 1000")
    parser.add_argument("-to", "--timeout", type=int, default=1, help="Solver time-out in minutes. Default: 1")
    parser.add_argument("--incumbent", type=str, default="off", choices=list(cluster_solve.INCUMBENT_MODES),
                        help="Greedy incumbents of every round's problems, computed on the GPU: cutoff = an objective bound for the solves; "
                             "fallback = also the round's isoform when a solve ends without a proven optimum (status INCUMBENT).  Default: off "
                             "(nothing changes)")
    parser.add_argument("--exact-small", type=int, default=0, choices=range(0, cluster_solve.EXACT_MAX_COLS + 1), metavar="N",
                        help="Problems of at most N columns (0 .. {}) are solved on the GPU by enumerating every column set: a proven optimum, the "
                             "smallest set at equal cost, and no solver call.  Default: 0 (nothing changes, no extra call).  {}".format(
                                 cluster_solve.EXACT_MAX_COLS, EXACT_HELP))
    parser.add_argument("--exact-masks", type=int, default=EXACT_MASKS, metavar="M",
                        help="Budget of a round's exact call: the sum of 2^columns over the problems it takes, smallest first; the rest go to the "
                             "solver.  Default: {}".format(EXACT_MASKS))
    parser.add_argument("--exact-bnb", type=int, default=0, choices=range(0, cluster_solve.BNB_MAX_COLS + 1), metavar="N",
                        help="Problems of more columns than --exact-small and at most N (0 .. {}) are searched on the GPU by branch and bound, "
                             "bounded by the greedy incumbents: a search that finishes is a proven optimum and no solver call; one that does "
                             "not hands the solver its best set as an incumbent.  Default: 0 (nothing changes, no extra call).  {}".format(
                                 cluster_solve.BNB_MAX_COLS, BNB_HELP))
    parser.add_argument("--bnb-nodes", type=int, default=BNB_NODES, metavar="M",
                        help="Budget of a round's branch and bound: the sum of tasks x node cap over the problems it takes, smallest first; the "
                             "rest go to the solver.  Default: {}".format(BNB_NODES))
    parser.add_argument("--exact-wide", type=int, default=0, choices=range(0, cluster_solve.BNB_WIDE_MAX_COLS + 1), metavar="N",
                        help="Problems of more columns than --exact-small and --exact-bnb and at most N (0 .. {}) whose tables fit the GPU's "
                             "on-chip memory are searched by the same branch and bound on column sets of several words, a wave a task; answers "
                             "are handled as --exact-bnb's.  Default: 0 (nothing changes, no extra call).  {}".format(
                                 cluster_solve.BNB_WIDE_MAX_COLS, WIDE_HELP))
    parser.add_argument("--wide-nodes", type=int, default=WIDE_NODES, metavar="M",
                        help="Budget of a round's wide branch and bound, as --bnb-nodes.  Default: {}".format(WIDE_NODES))
    parser.add_argument("--wide-passes", type=int, default=1, choices=range(1, WIDE_MAX_PASSES + 1), metavar="K",
                        help="Passes of a round's wide branch and bound (1 .. {}): beyond the first, the open subtrees of the tasks that stopped at "
                             "their node cap are searched as tasks of their own, bounded by the best set found so far, so that a launch stays "
                             "one node cap long.  Default: 1 (the single search, nothing changes).  {}".format(WIDE_MAX_PASSES, WIDE_PASSES_HELP))
    parser.add_argument("--device-rounds", action="store_true",
                        help="Keep every round's models on the GPU and read the isoforms of the problems --exact-small / --exact-bnb / "
                             "--exact-wide have answered out there; only the other problems are modelled on the host, for the solver.  Needs "
                             "--exact-small, --exact-bnb or --exact-wide.  Default: off (nothing changes).  {}".format(DEVICE_ROUNDS_HELP))
    parser.add_argument("-t", "--threads", type=int, default=1, help="Number of processes that solve (at most {})".format(MAX_WORKERS))
    parser.add_argument("-l", "--logs-dir", type=str, default=None, help="Directory path where logs will be outputted. Default: No log")
    parser.add_argument("-o", "--outdir", type=str, default="freddie_cluster/", help="Path to output directory. Default: freddie_cluster/")
    args = parser.parse_args(argv)
    assert args.recycle_model in recycle_models
    assert args.gap_offset >= 0
    assert args.epsilon >= 0
    assert args.timeout > 0
    assert args.threads > 0
    assert args.min_isoform_size >= 0
    assert args.max_rounds >= 0
    if args.exact_masks < 1:
        parser.error("--exact-masks must be at least 1")
    if args.bnb_nodes < 1:
        parser.error("--bnb-nodes must be at least 1")
    if args.wide_nodes < 1:
        parser.error("--wide-nodes must be at least 1")
    if args.device_rounds and not (args.exact_small > 0 or args.exact_bnb > 0 or args.exact_wide > 0):
        parser.error("--device-rounds needs --exact-small, --exact-bnb or --exact-wide: without them no problem is answered on the GPU")
    return args


def main(argv=None, make_context=None):
    """make_context: what opens the device context, cluster_prep.Context by default (a stand-in runs the command line without a GPU)."""
    import glob
    args = parse_args(argv)
    args.segment_dir = args.segment_dir.rstrip("/")
    settings = ilp_settings(args.recycle_model, args.epsilon, args.gap_offset, args.timeout, args.max_rounds, args.min_isoform_size, args.max_ilp,
                            args.incumbent, args.exact_small, args.exact_masks, args.exact_bnb, args.bnb_nodes, args.device_rounds, args.exact_wide, args.wide_nodes,
                            args.wide_passes)
    cluster_solve.check_settings(settings)
    jobs = []
    for contig in os.listdir(args.segment_dir):
        if not os.path.isdir("{}/{}".format(args.segment_dir, contig)):
            continue
        os.makedirs("{}/{}".format(args.outdir, contig), exist_ok=False)
        if args.logs_dir is not None:
            os.makedirs("{}/{}".format(args.logs_dir, contig), exist_ok=False)
        for path in glob.iglob("{}/{}/segment_*.tsv".format(args.segment_dir, contig)):
            jobs.append((contig, int(path[:-4].split("/")[-1].split("_")[-1]), path))
    pool = None
    if args.threads > 1:                                     # before the GPU is opened: the workers are forked without it and never touch it
        from multiprocessing import Pool
        pool = Pool(min(args.threads, MAX_WORKERS))
    try:
        ctx = (make_context or cluster_prep.Context)(0)
        try:
            results = cluster_files([j[2] for j in jobs], settings, ctx, pool=pool, threads=min(args.threads, MAX_WORKERS))
            for idx, ((contig, tint_id, _), (tints, logs)) in enumerate(zip(jobs, results)):       # written as the batches finish
                assert len(tints) == 1
                tint = tints[0]
                if args.logs_dir is not None:
                    os.makedirs("{}/{}/{}".format(args.logs_dir, contig, tint["id"]), exist_ok=True)
                    with open("{}/{}/{}/timeout.log".format(args.logs_dir, contig, tint["id"]), "w+") as log:
                        for line in logs[0]:
                            print("\t".join(map(str, line)), file=log)
                with open("{}/{}/cluster_{}_{}.tsv".format(args.outdir, contig, contig, tint_id), "w+") as out_file:
                    output_isoforms(tint, out_file)
                print("[freddie_cluster] Done with {}/{} tints ({:.1%})".format(idx + 1, len(jobs), (idx + 1) / len(jobs)))
        finally:
            ctx.close()
    finally:
        if pool is not None:
            pool.close()
            pool.join()
    return 0
