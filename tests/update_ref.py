"""numpy restatements of the updater as configured and of the scene log (include/pcr.h section A11), written from the
header's rules: `plan_rules` over a bank of C slots in tests/track_ref.py's array form, float32 operation for operation
(the GPU tests compare the kernel with it bit for bit), and `log_append` over a log kept as a dict of numpy columns.

`FAULTS` names three deliberate mistakes that `plan_rules(fault=...)` can make; tests/test_update_rules_cpu.py shows that the
golden file of the reference's own updater catches each of them.  `make_frame` draws one frame for a given bank state."""
import numpy as np

import track_ref as R

F = np.float32
OUTPUT, ACTIVE, DECOM = 1, 2, 4
KEEP, MISS = 0, 1
TABLE = ("out_valid", "out_ids", "out_labels", "out_scores", "out_boxes", "out_flags")
FAULTS = ("index_order_ids", "propagate_unmatched", "output_expired")
RULE_KEYS = ("match", "det_newborn", "det_false_positive", "track_false_positive", "track_false_negative")


def rule_word(cfg):
    return OUTPUT * bool(cfg["output"]) + ACTIVE * bool(cfg["active"]) + DECOM * bool(cfg["decom"])


def rules_from_config(update_config, det_names, trk_names):
    """-> dict(match_rule, det_rule, trk_rule, trk_kind) for the sorted decision names of a frame"""
    return dict(match_rule=rule_word(update_config["match"]),
                det_rule=[rule_word(update_config[k]) for k in det_names],
                trk_rule=[rule_word(update_config[k]) for k in trk_names],
                trk_kind=[MISS if k == "track_false_negative" else KEEP for k in trk_names])


def new_table(rows, W):
    return dict(out_valid=np.zeros(rows, np.int32), out_ids=np.full(rows, -1, np.int32),
                out_labels=np.full(rows, -1, np.int32), out_scores=np.zeros(rows, F), out_boxes=np.zeros((rows, W), F),
                out_flags=np.zeros(rows, np.int32))


def _free(st, s):
    st["ids"][s] = st["labels"][s] = -1
    st["lengths"][s] = 0


def plan_rules(st, track_to_det, det_to_track, det_labels, det_lengths, det_boxes, det_scores, det_decision,
               track_decision, rules, carry=None, frame_limit=10, replace_all=False, reset_on_match=False, fault=None):
    """-> (the new state, src (C,), det_slot (D,), det_id (D,), info (2,), the output table); `st` itself is left alone.
    The state's own info[0] is the number of dropped newborns, as track_ref.plan leaves it."""
    assert fault is None or fault in FAULTS
    old, st = st, R.copy_state(st)
    C, D, W = len(old["ids"]), len(det_labels), old["boxes"].shape[1]
    match_rule, det_rule, trk_rule, trk_kind = (rules[k] for k in ("match_rule", "det_rule", "trk_rule", "trk_kind"))
    dd, td = len(det_rule), len(trk_rule)
    for w in [match_rule] + list(det_rule) + list(trk_rule):
        assert not (w & ACTIVE and w & DECOM)
    table = new_table(C + D, W)
    src = np.full(C, -1, np.int32)
    det_slot, det_id = np.full(D, -1, np.int32), np.full(D, -1, np.int32)

    def put(row, ident, label, score, box, flags):
        table["out_valid"][row], table["out_ids"][row], table["out_labels"][row] = 1, ident, label
        table["out_scores"][row], table["out_boxes"][row], table["out_flags"][row] = score, box, flags

    def apply(rule, s, flags=0):
        if rule & OUTPUT:
            put(s, st["ids"][s], st["labels"][s], st["scores"][s], st["boxes"][s], flags | (1 if rule & DECOM else 0))
        if not rule & ACTIVE:
            _free(st, s)

    active = old["ids"] >= 0
    for s in np.nonzero(active)[0]:
        d, code = int(track_to_det[s]), int(track_decision[s])
        if (code == 0 and 0 <= d < D and det_labels[d] >= 0 and det_to_track[d] == s and det_decision[d] == 0):
            det_slot[d], det_id[d] = s, old["ids"][s]
            st["boxes"][s], st["scores"][s], st["labels"][s] = det_boxes[d], det_scores[d], det_labels[d]
            st["steps"][s] += 1
            if reset_on_match:
                st["misses"][s] = 0
            if replace_all or old["lengths"][s] <= det_lengths[d]:
                st["lengths"][s] = det_lengths[d]
                src[s] = d
            apply(match_rule, s)
            continue
        j = code - 1 if 1 <= code <= td else -1
        if j >= 0 and trk_kind[j] == KEEP:
            apply(trk_rule[j], s)
            continue
        miss = j >= 0 or fault == "propagate_unmatched"          # track_false_negative; anything else waits
        st["misses"][s] += 1
        if st["misses"][s] >= frame_limit:
            if fault == "output_expired" and j >= 0 and trk_rule[j] & OUTPUT:
                put(s, old["ids"][s], old["labels"][s], old["scores"][s], old["boxes"][s], 0)
            _free(st, s)
        elif miss:
            st["boxes"][s] = R.propagate_box(old["boxes"][s], carry)
            st["scores"][s] = F(old["scores"][s] * F(0.01))
            st["steps"][s] += 1
            if j >= 0:
                apply(trk_rule[j], s, flags=2)
            else:                                                # (the fault only: the branch the reference has commented out)
                put(s, st["ids"][s], st["labels"][s], st["scores"][s], st["boxes"][s], 2)

    # new tracks: numbered by decision, then by index; the ACTIVE ones take the slots that were free, in that same order
    order = [(i, d) for i in range(dd) for d in range(D) if det_labels[d] >= 0 and det_decision[d] == 1 + i]
    if fault == "index_order_ids":
        order.sort(key=lambda e: e[1])
    free = list(np.nonzero(~active)[0])
    dropped = 0
    for k, (i, d) in enumerate(order):
        ident = old["next_id"][0] + k
        det_id[d] = ident
        rule = det_rule[i]
        if rule & ACTIVE and free:
            s = free.pop(0)
            st["ids"][s], st["steps"][s], st["misses"][s] = ident, 1, 0
            st["labels"][s], st["lengths"][s] = det_labels[d], det_lengths[d]
            st["boxes"][s], st["scores"][s] = det_boxes[d], det_scores[d]
            src[s], det_slot[d] = d, s
            if rule & OUTPUT:
                put(s, ident, det_labels[d], det_scores[d], det_boxes[d], 0)
        else:
            dropped += bool(rule & ACTIVE)
            if rule & OUTPUT:
                put(C + d, ident, det_labels[d], det_scores[d], det_boxes[d], 1 if rule & DECOM else 0)
    st["next_id"][0] = old["next_id"][0] + len(order)
    st["info"][0] = dropped
    info = np.array([dropped, int(table["out_valid"].sum())], np.int32)
    return st, src, det_slot, det_id, info, table


# ---- the scene log ----------------------------------------------------------------------------------------------------
def new_log(rows_max, W):
    return dict(frame=np.zeros(rows_max, np.int32), id=np.zeros(rows_max, np.int32), label=np.zeros(rows_max, np.int32),
                flags=np.zeros(rows_max, np.int32), score=np.zeros(rows_max, F), box=np.zeros((rows_max, W), F),
                cursor=np.zeros(1, np.int32), dropped=np.zeros(1, np.int32), frame_no=np.zeros(1, np.int32))


def log_append(log, table):
    """-> the new log; `log` itself is left alone"""
    log = {k: v.copy() for k, v in log.items()}
    rows_max = len(log["frame"])
    cursor = int(log["cursor"][0])
    if not 0 <= cursor <= rows_max:
        cursor = rows_max
    rows = np.nonzero(table["out_valid"] != 0)[0]
    written = min(len(rows), rows_max - cursor)
    for k, r in enumerate(rows[:written]):
        at = cursor + k
        log["frame"][at], log["id"][at], log["label"][at] = log["frame_no"][0], table["out_ids"][r], table["out_labels"][r]
        log["flags"][at], log["score"][at], log["box"][at] = table["out_flags"][r], table["out_scores"][r], table["out_boxes"][r]
    log["cursor"][0] = cursor + written
    log["dropped"][0] += len(rows) - written
    log["frame_no"][0] += 1
    return log


def log_records(log):
    n = int(log["cursor"][0])
    return {k: log[k][:n] for k in ("frame", "id", "label", "flags", "score", "box")}


# ---- frames ---------------------------------------------------------------------------------------------------------------
def make_frame(g, st, D, W, dd, td, junk=True, p_match=0.5, p_valid=0.85, p_new=0.7):
    """one frame for the bank state `st`: track_ref.make_frame's detections and maps (with their entries that the rules
    must ignore), and decision codes that agree with the intended pairs -- plus, with junk, codes out of range, matched
    codes without a pair and decision codes on paired objects"""
    fr = R.make_frame(g, st, D, W, masks=False, junk=junk, p_match=p_match, p_valid=p_valid)
    C = len(st["ids"])
    ddec = np.where(g.random(D) < p_new, 1 + g.integers(0, max(dd, 1), D), 1 + dd).astype(np.int32)
    if dd == 0:
        ddec[:] = 1
    tdec = np.where(g.random(C) < 0.7, 1 + g.integers(0, max(td, 1), C), 1 + td).astype(np.int32)
    if td == 0:
        tdec[:] = 1
    for s, d in fr["intended"]:
        tdec[s], ddec[d] = 0, 0
    if junk:
        for a, n in ((ddec, D), (tdec, C)):
            for i in range(n):
                u = g.random()
                if u < 0.06:
                    a[i] = [-1, 9, 1 << 20, -(1 << 30)][int(g.integers(0, 4))]
                elif u < 0.12:
                    a[i] = 0 if a[i] != 0 else 1               # a matched code without a pair, a decision on a paired one
    fr["det_decision"], fr["track_decision"] = ddec, tdec
    return fr


def plan_frame(st, fr, rules, **args):
    return plan_rules(st, fr["track_to_det"], fr["det_to_track"], fr["labels"], fr["lengths"], fr["boxes"], fr["scores"],
                      fr["det_decision"], fr["track_decision"], rules, **args)


def random_rules(g, dd, td):
    """rule words and kinds for dd / td decisions: any of the five words without ACTIVE | DECOM"""
    words = [0, OUTPUT, ACTIVE, OUTPUT | ACTIVE, DECOM, OUTPUT | DECOM]
    pick = lambda: words[int(g.integers(0, len(words)))]
    return dict(match_rule=[OUTPUT | ACTIVE, ACTIVE, OUTPUT | DECOM][int(g.integers(0, 3))],
                det_rule=[pick() for _ in range(dd)], trk_rule=[pick() for _ in range(td)],
                trk_kind=[int(g.integers(0, 2)) for _ in range(td)])
