"""The tracker frame behind `ReIDNet.associate` and `ReIDNet.track_step`: what a decisions= dict means, the assignment
(whole or class by class), and the two chains of launches.  Of the model a frame uses forward_inference_boxes and
match_gallery only; everything else is pcr_amd/associate.py, tracks.py, truth.py and identity.py.  The functions take the
model as their first argument, as `retrieval.evaluate_retrieval` does; the contracts and the keyword defaults are on the
model's methods, which hand their arguments over as they got them (cost_args as a dict)."""
import torch

from . import _lib as L
from . import associate as A
from . import identity as ID
from . import tracks as TR
from . import truth as TU


def decision_set(decisions, T, D, cost_args, who, M=None):
    """decisions=dict(detection=(names...), tracking=(names...), det_values=(dd, D) or None, track_values=(td, T) or
    None, kind="margin", reduce=False) -> what associate_decisions takes.  The names are sorted, as the reference sorts
    them (trackers/deprecated/virtual_tracker.py:114-115), and the rows of det_values / track_values follow the sorted
    order; None values are zeros.  det_values of width M < D (track_step's padding) are zero-padded."""
    if not isinstance(decisions, dict) or set(decisions) - {"detection", "tracking", "det_values", "track_values", "kind",
                                                            "reduce"}:
        raise L.PcrError("%s: decisions must be dict(detection=, tracking=, det_values=, track_values=, kind=, reduce=)"
                         % who)
    if "track_miss" in cost_args or "det_new" in cost_args:
        raise L.PcrError("%s: track_miss / det_new belong to the one-decision matrix; with decisions= the values are "
                         "det_values / track_values" % who)
    det_names, trk_names = sorted(decisions.get("detection", ())), sorted(decisions.get("tracking", ()))
    dev = torch.device("cuda", torch.cuda.current_device())
    values = []
    for names, v, n, key in ((det_names, decisions.get("det_values"), D, "det_values"),
                             (trk_names, decisions.get("track_values"), T, "track_values")):
        if v is None:
            v = torch.zeros((len(names), n), dtype=torch.float32, device=dev)
        v = L.tensor(v, who, "decisions[%r]" % key, torch.float32, copy=True)
        if key == "det_values" and M is not None and v.dim() == 2 and v.shape[1] == M and M < n:
            v = torch.cat([v, v.new_zeros((v.shape[0], n - M))], dim=1)
        values.append(L.tensor(v, who, "decisions[%r]" % key, torch.float32, shape=(len(names), n)))
    L.require_cuda(*values)
    return dict(det_names=det_names, trk_names=trk_names, det_values=values[0], trk_values=values[1],
                kind=decisions.get("kind", "margin"), reduce=bool(decisions.get("reduce", False)),
                born=det_names.index("det_newborn") if "det_newborn" in det_names else -1,
                kill=trk_names.index("track_false_positive") if "track_false_positive" in trk_names else -1)


def assign(cost, T, D, dd, td, reduce, by_class):
    """linear_assignment over cost, or -- by_class = (track_labels, det_labels, num_classes) -- the block rule: the ids
    from the labels on the device, one wave per class (linear_assignment_blocks) and the solver's one word as the
    maximum over the blocks -> (col4row (R,), row4col (C,), info (1,)), block_info (G,) or None"""
    if by_class is None:
        col4row, row4col, info = A.linear_assignment(cost)
        return (col4row[0], row4col[0], info), None
    row_block, col_block, G = A.association_blocks(by_class[0], by_class[1], T, D, dd, td, num_classes=by_class[2],
                                                   reduce=reduce)
    col4row, row4col, block_info = A.linear_assignment_blocks(cost, row_block, col_block, G)
    return (col4row, row4col, block_info.amax(dim=0, keepdim=True)), block_info


def assign_one(cost, T, D, by_class):
    """assign over association_cost's one-decision matrix, the columns >= D and the rows >= T (the miss / new diagonals)
    read as -1 -> track_to_det (T,), det_to_track (D,), info (1,), block_info or None"""
    (col4row, row4col, info), block_info = assign(cost, T, D, 1, 1, False, by_class)
    c, r = col4row[:T], row4col[:D]
    return torch.where(c < D, c, torch.full_like(c, -1)), torch.where(r < T, r, torch.full_like(r, -1)), info, block_info


def match_across(model, feats, xyz, pairs, offset, count):
    """match_gallery over a gallery [a | b] of `offset` rows of a followed by b's, for pairs (row of a, row of b)"""
    gallery_pairs = torch.stack([pairs[:, 0], pairs[:, 1] + offset], dim=1)
    return model.match_gallery(feats, xyz, gallery_pairs, count=count).contiguous()


def associate_decisions(logits, pairs, count, T, D, ds, dist, cost_args, by_class=None):
    """the matrix for the decision set ds, its assignment and the decode (pcr_amd/associate.py) -> the entries that
    associate / track_step return"""
    dd, td = len(ds["det_names"]), len(ds["trk_names"])
    R, C = A.multi_shape(T, D, dd, td, ds["reduce"])
    if not L.load().pcr_lsa_ok(1, R, C):
        raise L.PcrError("decisions: the (%d, %d) matrix is beyond linear_assignment (PCR_LSA_MAX)" % (R, C))
    out = A.association_cost_multi(logits, pairs, count, T, D, ds["det_values"], ds["trk_values"], kind=ds["kind"],
                                   reduce=ds["reduce"], dist=dist, **cost_args)
    cost, choices = (out[0], (out[1], out[2])) if ds["reduce"] else (out, None)
    assignment, block_info = assign(cost, T, D, dd, td, ds["reduce"], by_class)
    dec = A.decode_assignment(cost, assignment, T, D, dd, td, fill=cost_args.get("fill", 10000.0), choices=choices,
                              born_decision=ds["born"], kill_decision=ds["kill"])
    return dict(track_to_det=dec["track_to_det"], det_to_track=dec["det_to_track"], cost=cost, info=assignment[2],
                det_decision=dec["det_decision"], track_decision=dec["track_decision"], born=dec["born"],
                kill=dec["kill"], decode_info=dec["info"], **({} if block_info is None else {"block_info": block_info}))


def associate(model, track_feats, track_xyz, track_labels, track_lengths, det_feats, det_xyz, det_labels, det_lengths,
              min_points, num_classes, cap, live_only, decisions, by_class, cost_args):
    """ReIDNet.associate, which has the contract"""
    L.require_cuda(track_feats, track_xyz, det_feats, det_xyz)
    T, D = track_feats.shape[0], det_feats.shape[0]
    ds = None if decisions is None else decision_set(decisions, T, D, cost_args, "associate")
    pairs, count = A.compare_pairs(track_labels, det_labels, track_lengths, det_lengths, min_points=min_points,
                                   num_classes=num_classes, cap=cap)
    dev = track_feats.device
    blocks = (track_labels, det_labels, num_classes) if by_class else None
    if T == 0 or D == 0:
        # an empty side has nothing to match.  One decision: no assignment either, the list is handed back as it is with
        # logits nobody wrote.  A decision set: no special case, the side that is there still takes its decisions
        if ds is None:
            empty = {"block_info": torch.zeros((num_classes + 1,), dtype=torch.int32, device=dev)} if by_class else {}
            return dict(track_to_det=torch.full((T,), -1, dtype=torch.int32, device=dev),
                        det_to_track=torch.full((D,), -1, dtype=torch.int32, device=dev), pairs=pairs, count=count,
                        logits=torch.empty((pairs.shape[0],), dtype=torch.float32, device=dev), cost=None,
                        info=torch.zeros((1,), dtype=torch.int32, device=dev), **empty)
        pairs, logits = pairs[:0], torch.empty((0,), dtype=torch.float32, device=dev)
    else:
        logits = match_across(model, torch.cat([track_feats, det_feats], dim=0), torch.cat([track_xyz, det_xyz], dim=0),
                              pairs, T, count if live_only else None)                      # detections follow the tracks
    if ds is not None:
        dist = cost_args.pop("dist", None)
        return dict(pairs=pairs, count=count, logits=logits,
                    **associate_decisions(logits, pairs, count, T, D, ds, dist, cost_args, by_class=blocks))
    cost = A.association_cost(logits, pairs, count, T, D, **cost_args)
    t2d, d2t, info, block_info = assign_one(cost, T, D, blocks)
    return dict(track_to_det=t2d, det_to_track=d2t, pairs=pairs, count=count, logits=logits, cost=cost, info=info,
                **({} if block_info is None else {"block_info": block_info}))


def _frame_arguments(bank, sweep, boxes, labels, scores, born, kill, propagate, truth, force_truth, decisions,
                     update_config, log, cost_args):
    """every rule on track_step's arguments, in one place and before the frame's first launch: which of truth / identity /
    decisions / update_config / log / born / kill / propagate / force_truth go together and over which bank, the
    detections' shapes, and whether the assignment's matrix is within linear_assignment.  (The decision set is made here
    because the last rules read it: a zero fill or the padding of its values is the only device work.)
    -> boxes (M, W), scores (M,) as float32 tensors, the decision set or None, the UpdateRules or None"""
    if truth is None and force_truth:
        raise L.PcrError("track_step: force_truth needs truth=")
    if truth is not None:
        book = truth.get("book") if isinstance(truth, dict) else None
        if not isinstance(book, TU.TruthBook) or book.bank is not bank:
            raise L.PcrError("track_step: truth['book'] must be a pcr_amd.truth.TruthBook made over this bank")
        identity = truth.get("identity")
        if identity is not None and (not isinstance(identity, ID.IdentityBook) or identity.book is not book):
            raise L.PcrError("track_step: truth['identity'] must be a pcr_amd.identity.IdentityBook made over "
                             "truth['book']")
    if not isinstance(bank, TR.TrackBank):
        raise L.PcrError("track_step: bank must be a pcr_amd.tracks.TrackBank")
    if decisions is not None and (born is not None or kill is not None):
        raise L.PcrError("track_step: with decisions= the born / kill masks come from the decoded decisions; pass one or "
                         "the other")
    C, D, W = bank.capacity, bank.max_dets, bank.box_width
    if update_config is not None:
        if decisions is None:
            raise L.PcrError("track_step: update_config applies to decoded decisions; pass decisions= with it")
        if born is not None or kill is not None or not propagate or force_truth:
            raise L.PcrError("track_step: update_config cannot be combined with born= / kill=, propagate= or "
                             "force_truth=: the rules decide what is born, dropped and propagated")
    if log is not None:
        if update_config is None:
            raise L.PcrError("track_step: log= records the output table; pass update_config= with it")
        if not isinstance(log, TR.SceneLog) or (log.rows_per_frame, log.box_width) != (C + D, W):
            raise L.PcrError("track_step: log must be a pcr_amd.tracks.SceneLog of %d rows per frame and box width %d"
                             % (C + D, W))
    boxes = L.tensor(boxes, "track_step", "boxes", torch.float32, shape=(None, W), copy=True)
    M = boxes.shape[0]
    L.require(M <= D, "track_step", "boxes must be (M <= %d, %d), got %s", D, W, tuple(boxes.shape))
    scores = L.tensor(scores, "track_step", "scores", torch.float32, shape=(M,), copy=True)
    L.require(isinstance(labels, torch.Tensor) and labels.shape == (M,), "track_step", "labels must be (M,)")
    L.require_cuda(sweep, boxes, labels, scores)
    ds = None if decisions is None else decision_set(decisions, C, D, cost_args, "track_step", M=M)
    rules = None if update_config is None else TR.UpdateRules(update_config, ds["det_names"], ds["trk_names"])
    if ds is None and not L.load().pcr_lsa_ok(1, C + D, C + D):
        raise L.PcrError("track_step: capacity + max_dets = %d is beyond linear_assignment (PCR_LSA_MAX)" % (C + D))
    if ds is not None:
        if not L.load().pcr_lsa_ok(1, *A.multi_shape(C, D, len(ds["det_names"]), len(ds["trk_names"]), ds["reduce"])):
            raise L.PcrError("track_step: the decisions' matrix for capacity %d and max_dets %d is beyond "
                             "linear_assignment (PCR_LSA_MAX)" % (C, D))
    return boxes, scores, ds, rules


def track_step(model, bank, sweep, boxes, labels, scores, carry, carry_inv, min_points, num_classes, cap, n, crop_args,
               born, kill, frame_limit, replace_all, reset_on_match, propagate, suppress_threshold, live_only, truth,
               force_truth, decisions, by_class, update_config, log, cost_args):
    """ReIDNet.track_step, which has the contract"""
    boxes, scores, ds, rules = _frame_arguments(bank, sweep, boxes, labels, scores, born, kill, propagate, truth,
                                                force_truth, decisions, update_config, log, cost_args)
    book = None if truth is None else truth["book"]
    identity = None if truth is None else truth.get("identity")
    C, D, W, M = bank.capacity, bank.max_dets, bank.box_width, boxes.shape[0]
    labels = labels.to(torch.int32)
    if M < D:                                   # padding: a box of size zero holds no point, label -1 joins nothing
        boxes = torch.cat([boxes, boxes.new_zeros((D - M, W))], dim=0)
        labels = torch.cat([labels, labels.new_full((D - M,), -1)], dim=0)
        scores = torch.cat([scores, scores.new_zeros((D - M,))], dim=0)
        if born is not None and born.shape == (M,):
            born = torch.cat([born, born.new_zeros((D - M,))], dim=0)
    boxes, labels, scores = boxes.contiguous(), labels.contiguous(), scores.contiguous()
    xyz, feats, lengths = model.forward_inference_boxes(sweep, boxes[:, :7].contiguous(), n=n, **(crop_args or {}))
    if tuple(feats.shape[1:]) != bank.feat_shape or tuple(xyz.shape[1:]) != (bank.feat_shape[1], 3):
        raise L.PcrError("track_step: the encoder returns features %s, the bank was made for %s"
                         % (tuple(feats.shape[1:]), bank.feat_shape))
    bank.det_feats.copy_(feats)
    bank.det_xyz.copy_(xyz)
    dist = bank.distances(boxes, carry_inv)
    pairs, count = A.compare_pairs(bank.labels, labels, bank.lengths, lengths, min_points=min_points,
                                   num_classes=num_classes, cap=cap)
    logits = match_across(model, bank.gallery, bank.gallery_xyz, pairs, C,
                          count if live_only else None)                                    # detections follow the bank's rows
    blocks = (bank.labels, labels, num_classes) if by_class else None
    decoded = {}
    if ds is not None:
        decoded = associate_decisions(logits, pairs, count, C, D, ds, dist if ds["kind"] == "margin" else None,
                                      cost_args, by_class=blocks)
        t2d, d2t, cost, info = (decoded.pop(k) for k in ("track_to_det", "det_to_track", "cost", "info"))
        born, kill = decoded["born"], decoded["kill"]
    else:
        cost = A.association_cost(logits, pairs, count, C, D, dist=dist, **cost_args)
        t2d, d2t, info, block_info = assign_one(cost, C, D, blocks)
        if block_info is not None:
            decoded["block_info"] = block_info
    decisions, truth_out = (t2d, d2t), {}
    if truth is not None:
        book.match(boxes, labels, truth)
        truth_out = book.decide(decisions, labels, born=born, kill=kill, forced=force_truth)
        if force_truth:
            decisions, born, kill = book.forced()
    dets = dict(labels=labels, lengths=lengths, boxes=boxes, scores=scores)
    if rules is not None:
        det_slot, det_id, bank_info, table = bank.update_rules(
            decisions, dets, decoded["det_decision"], decoded["track_decision"], rules, carry=carry,
            frame_limit=frame_limit, replace_all=replace_all, reset_on_match=reset_on_match)
        decoded = dict(decoded, **table)
        if log is not None:
            log.append(table)
    else:
        det_slot, det_id, bank_info = bank.update(decisions, dets, born=born, kill=kill, carry=carry,
                                                  frame_limit=frame_limit, replace_all=replace_all,
                                                  reset_on_match=reset_on_match, propagate=propagate)
    if suppress_threshold is not None:
        bank.suppress(suppress_threshold)
    if truth is not None:
        book.record(det_slot, det_id)
        if identity is not None:
            identity.record(det_id)
    return dict(track_to_det=t2d, det_to_track=d2t, pairs=pairs, count=count, logits=logits, cost=cost, info=info,
                det_slot=det_slot, det_id=det_id, bank_info=bank_info, dist=dist, lengths=lengths, **decoded, **truth_out)
