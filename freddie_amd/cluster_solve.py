"""The solve of one round's ILP (py/freddie_cluster.py run_ilp :347-592 with K = 2) behind a narrow interface: a plain callable
``solve(model, settings) -> (status, x, e)``.  The backend here is HiGHS through scipy.optimize.milp; where a Gurobi licence exists a
backend for it is another callable of the same shape.  Optimal solutions of equal cost may differ between solvers: HiGHS breaks ties
its own way, so the isoforms of a round can differ from Gurobi's where the optimum is not unique.

With K = 2 (isoform 0 is the garbage isoform, isoform 1 the round's) the reference's model is, over the remaining reps ("columns")
and the informative segments:
  x_i  binary   rep i is in the round's isoform (R2I[i][1]; R2I[i][0] = 1 - x_i)
  e_j  binary   segment j is in the isoform: the OR of the x_i over the reps that cover it (E2I_C1, a max constraint :440-445)
                    e_j >= x_i for every support entry, e_j <= sum of those x_i (no entry: e_j = 0)
  o_ij in [0,1] rep i is in, j is in, and C[i][j] = 1: a correction (OBJ_C1 :530-534), cost 1;  o_ij >= x_i + e_j - 1
  G_g  = sum of len_j e_j over the group's segments (GAPI_C1 :474-481), and per (column, gap of length l) the two big-M rows
                    (1 - epsilon) G_g - offset - (1 - x_i) MAX_LG <= l   (:482-489)
                    (1 + epsilon) G_g + offset + (1 - x_i) MAX_LG >= l   (:490-497)
  x_a + x_b <= 1 per incompatible pair (:505-511);  the garbage cost on 1 - x_i (:544).
``model`` = cluster_prep.round_model() of the problem plus ``garbage`` (a cost per column) and ``max_lg`` (the tint's summed segment
lengths).  The relative recycle model needs E2I_min and the reference's preprocess_ilp() sets no garbage cost for it: refused."""
import numpy as np

OPTIMAL, NO_SOLUTION = "OPTIMAL", "NO_SOLUTION"
RECYCLE_MODELS = ("constant", "exons", "introns")


def check_settings(settings):
    if settings["recycle_model"] not in RECYCLE_MODELS:
        raise ValueError("recycle model %r: the solve supports %s (relative needs E2I_min and has no garbage cost in the reference either)"
                         % (settings["recycle_model"], ", ".join(RECYCLE_MODELS)))


def build_rows(model, settings):
    """(cost, A as (data, rows, cols), lower, upper, upper bounds of the variables, constant of the objective): variables are the R
    columns' x, then the e of inf_seg, then one o per correction term."""
    R, inf_seg = model["n_cols"], model["inf_seg"]
    E = len(inf_seg)
    e_of = {j: R + k for k, j in enumerate(inf_seg)}
    terms = [(c, j) for c, segs in enumerate(model["corrections"]) for j in segs]
    n = R + E + len(terms)
    cost = np.zeros(n)
    cost[:R] = -np.asarray(model["garbage"], float)
    cost[R + E:] = 1.0
    ub = np.ones(n)
    data, rows, cols, lo, hi = [], [], [], [], []

    def row(entries, lower, upper):
        r = len(lo)
        for col, v in entries:
            data.append(v); rows.append(r); cols.append(col)
        lo.append(lower); hi.append(upper)

    for k, support in enumerate(model["support"]):
        if not support:
            ub[R + k] = 0.0
            continue
        for c in support:
            row([(R + k, 1.0), (c, -1.0)], 0.0, np.inf)
        row([(R + k, 1.0)] + [(c, -1.0) for c in support], -np.inf, 0.0)
    for t, (c, j) in enumerate(terms):
        row([(R + E + t, 1.0), (c, -1.0), (e_of[j], -1.0)], -1.0, np.inf)
    eps, off, big = settings["epsilon"], settings["offset"], model["max_lg"]
    for c, g, l in model["gap_rows"]:
        segs = model["group_segs"][g]
        row([(e_of[j], (1.0 - eps) * ln) for j, ln in segs] + [(c, float(big))], -np.inf, l + off + big)
        row([(e_of[j], (1.0 + eps) * ln) for j, ln in segs] + [(c, -float(big))], l - off - big, np.inf)
    for a, b in model["pairs"]:
        row([(a, 1.0), (b, 1.0)], -np.inf, 1.0)
    return cost, (data, rows, cols), np.array(lo), np.array(hi), ub, float(sum(model["garbage"]))


def solve_round(model, settings):
    """(status, x, e): status OPTIMAL only for a proven optimum within timeout minutes (anything else is NO_SOLUTION, as :591-592),
    x a 0 / 1 per column, e a 0 / 1 per informative segment (beside model['inf_seg']).  The relative gap is 0: costs are multiples of
    0.5 and a relative gap would accept a worse isoform."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import csr_matrix
    check_settings(settings)
    R, E = model["n_cols"], len(model["inf_seg"])
    if R == 0:
        return OPTIMAL, [], [0] * E
    cost, (data, rows, cols), lo, hi, ub, _ = build_rows(model, settings)
    n = cost.size
    integrality = np.zeros(n)
    integrality[:R + E] = 1
    constraints = [LinearConstraint(csr_matrix((data, (rows, cols)), shape=(lo.size, n)), lo, hi)] if lo.size else []
    res = milp(cost, integrality=integrality, bounds=Bounds(np.zeros(n), ub), constraints=constraints,
               options=dict(time_limit=settings["timeout"] * 60, mip_rel_gap=0.0, disp=False))
    if res.status != 0 or res.x is None:
        return NO_SOLUTION, None, None
    return OPTIMAL, [int(v > 0.5) for v in res.x[:R]], [int(v > 0.5) for v in res.x[R:R + E]]


def round_cost(model, x, e):
    """The objective's value of a solution: the chosen reps' corrections and the others' garbage costs."""
    on = {j for j, v in zip(model["inf_seg"], e) if v}
    return (sum(g for g, v in zip(model["garbage"], x) if not v) +
            sum(1 for c, segs in enumerate(model["corrections"]) if x[c] for j in segs if j in on))
