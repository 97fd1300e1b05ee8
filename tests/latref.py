"""N-best and marginals over an explicit lattice, in plain Python -- TEST INFRASTRUCTURE ONLY.

Written from the contract in include/vibrato_hip.h (the header comments of vbt_tokenize_nbest and vbt_tokenize_marginal), not from
nbest.hip / marginal.hip: integer costs as Python ints, lists for the per-node entries, the `decimal` module for the sums.  A lattice is
what pyref.PyTokenizer.lattice() returns: {"num_chars", "nodes", "eos_from"}, the nodes in lattice order, each naming the end position its
predecessors are taken from (start_node) and its own slot in its end list; slot 0 of end list 0 is BOS (right id 0, cost 0), EOS has
left id 0 and connects from end list `eos_from`.  `conn(right_id, left_id)` is the connection cost.  Slow by design, small inputs only.
"""
import decimal

BOS = -1  # index of BOS where a node index is expected


def _wrap_i32(x):
    return ((x + 2**31) % 2**32) - 2**31


def end_lists(lat):
    """ends[p] = node indices (BOS first in ends[0]) in insertion order, checked against the nodes' own slots"""
    ends = [[] for _ in range(lat["num_chars"] + 1)]
    ends[0].append(BOS)
    for i, nd in enumerate(lat["nodes"]):
        assert nd["slot"] == len(ends[nd["end"]]) and nd["start_node"] <= nd["start_word"] < nd["end"]
        ends[nd["end"]].append(i)
    return ends


def num_steps(lat):
    """sweep steps: one per start position that inserted nodes, + EOS"""
    return len({nd["start_word"] for nd in lat["nodes"]}) + 1


def kbest(lat, conn, k):
    """The k cheapest paths: [(path_cost, [(start_char, end_char, start_byte, end_byte, word_idx, total_cost_along_path)])].  Every node
    keeps its k best (cost, (predecessor, rank of the predecessor's entry)); a list is the merge of the predecessors' lists in the
    contract's order: lower cost first; on equal cost the predecessor inserted later into the end list first, then the lower rank of
    its entry (the comparison from EOS backwards, applied recursively).  Costs wrap to i32 entry by entry.  An empty sentence has no
    path, a sentence without nodes (skipped spaces only) one path of no tokens."""
    if lat["num_chars"] == 0:
        return []
    nodes, ends = lat["nodes"], end_lists(lat)
    entries = []  # per node: [(cost, (pred, rank))]
    bos = [(0, None)]

    def merge(preds, left):
        offers = []
        for slot, p in enumerate(preds):
            right = 0 if p == BOS else nodes[p]["right"]
            c = conn(right, left)
            for rank, (cost, _) in enumerate(bos if p == BOS else entries[p]):
                offers.append((_wrap_i32(cost + c), -slot, rank, p))
        offers.sort()
        return [(cost, (p, rank)) for cost, _, rank, p in offers[:k]]

    for nd in nodes:
        entries.append([(_wrap_i32(cost + nd["wcost"]), back) for cost, back in merge(ends[nd["start_node"]], nd["left"])])
    paths = []
    for cost, back in merge(ends[lat["eos_from"]], 0):
        recs = []
        while back[0] != BOS:
            nd = nodes[back[0]]
            total, prev = entries[back[0]][back[1]]
            recs.append((nd["start_word"], nd["end"], nd["start_byte"], nd["end_byte"], (nd["lex"] << 30) | nd["wid"], total))
            back = prev
        recs.reverse()
        paths.append((cost, recs))
    return paths


_CTX = decimal.Context(prec=80, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN, rounding=decimal.ROUND_HALF_EVEN)


def marginals(lat, conn, T):
    """Forward-backward with 80-digit decimals: {"log_z": Decimal, "prob": [Decimal per node], "max_abs_alpha": float, "steps": int}.
    The weight of a path is exp(-cost / T) with cost the exact integer sum (nothing wraps); the sweeps run on the weights themselves
    (the decimal exponent has 18 digits, nothing under- or overflows), one Decimal.exp per distinct integer cost and one Decimal.ln
    for log Z.  Dead ends get probability 0.  A lattice without nodes, or with no path to EOS, gives log_z = 0 and every prob 0.
    max_abs_alpha = the largest |log forward weight| over the nodes and EOS, steps = num_steps(): what a float64 error bound needs."""
    nodes, ends = lat["nodes"], end_lists(lat)
    zero, one = decimal.Decimal(0), decimal.Decimal(1)
    if not nodes:
        return {"log_z": zero, "prob": [], "max_abs_alpha": 0.0, "steps": num_steps(lat)}
    t = decimal.Decimal(T)  # exact: a float is a binary fraction
    cache = {}

    def w(cost):
        if cost not in cache:
            cache[cost] = _CTX.exp(_CTX.divide(decimal.Decimal(-cost), t))
        return cache[cost]

    def right_of(p):
        return 0 if p == BOS else nodes[p]["right"]

    mul, add = _CTX.multiply, _CTX.add
    alpha = []  # summed weight of the partial paths BOS -> node, the node's word cost included
    for nd in nodes:
        s = zero
        for p in ends[nd["start_node"]]:
            s = add(s, mul(one if p == BOS else alpha[p], w(conn(right_of(p), nd["left"]))))
        alpha.append(mul(s, w(nd["wcost"])))
    z = zero
    for p in ends[lat["eos_from"]]:
        z = add(z, mul(alpha[p] if p != BOS else one, w(conn(right_of(p), 0))))
    # beta of a node = summed weight of the partial paths node -> EOS (its own word cost excluded).  The successors of an end list are
    # the nodes whose start_node names it; an end list is the predecessor list of whole steps, so beta is computed per end list entry.
    followers = [[] for _ in ends]
    for i, nd in enumerate(nodes):
        followers[nd["start_node"]].append(i)
    beta = [zero] * len(nodes)
    for pos in range(lat["num_chars"], 0, -1):
        for p in ends[pos]:
            s = w(conn(nodes[p]["right"], 0)) if pos == lat["eos_from"] else zero
            for c in followers[pos]:
                if beta[c] != zero:
                    s = add(s, mul(mul(w(conn(nodes[p]["right"], nodes[c]["left"])), w(nodes[c]["wcost"])), beta[c]))
            beta[p] = s
    if z == zero:
        return {"log_z": zero, "prob": [zero] * len(nodes), "max_abs_alpha": 0.0, "steps": num_steps(lat)}
    low = decimal.Context(prec=20, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
    max_abs_alpha = max(abs(float(low.ln(a))) for a in alpha + [z])
    return {"log_z": _CTX.ln(z), "prob": [_CTX.divide(mul(a, b), z) for a, b in zip(alpha, beta)], "max_abs_alpha": max_abs_alpha,
            "steps": num_steps(lat)}


def enumerate_paths(lat, conn, limit=10 ** 5):
    """Every path BOS -> EOS by depth-first search: [(exact integer cost, [node indices], [running exact cost per node])]; asserts
    that there are fewer than `limit`.  The anchor of kbest() and marginals() that shares nothing with them but end_lists()."""
    nodes, ends = lat["nodes"], end_lists(lat)
    if lat["num_chars"] == 0:
        return []
    followers = [[] for _ in ends]
    for i, nd in enumerate(nodes):
        followers[nd["start_node"]].append(i)
    paths = []

    def walk(pos, slot_right, total, seq, totals):
        if pos == lat["eos_from"]:
            paths.append((total + conn(slot_right, 0), seq, totals))
            assert len(paths) < limit
        for c in followers[pos]:
            nd = nodes[c]
            t = total + conn(slot_right, nd["left"]) + nd["wcost"]
            walk(nd["end"], nd["right"], t, seq + [c], totals + [t])

    walk(0, 0, 0, [], [])
    return paths


def count_paths(lat):
    """the number of paths BOS -> EOS, by an integer sweep"""
    if lat["num_chars"] == 0:
        return 0
    reach = [0] * (lat["num_chars"] + 1)
    reach[0] = 1
    for nd in lat["nodes"]:
        reach[nd["end"]] += reach[nd["start_node"]]
    return reach[lat["eos_from"]]
