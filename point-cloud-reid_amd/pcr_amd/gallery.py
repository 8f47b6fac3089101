"""The pair-list matcher behind `ReIDNet.match_gallery` for the attention heads: every object's key/value state is made
once, then the list is walked in passes of `model.GALLERY_CHUNK` pairs.  `match_pairs` is the one driver; the symmetric
head (xcorr_eff / point-cat / both) and the one-way heads (xcorr-baseline, xcorr) differ in the body of a pass only.
The functions take the model as their first argument, as `retrieval.evaluate_retrieval` does; the documented entry point
and the dispatch on match_type stay on the model."""
import torch

from . import _lib as L


def pair_count(count):
    """the count= of match_gallery / match_embeddings: None, or a (1,) int32 device tensor -> None or that, (1,) contiguous"""
    if count is None:
        return None
    L.require_cuda(count)
    if count.dtype != torch.int32 or count.numel() != 1:
        raise L.PcrError("match_gallery: count must be a (1,) int32 device tensor")
    return count.reshape(1).contiguous()


def _chunk_symmetric(model, p1, p2, h, xyz, state, i, j, live, dead_value):
    """one pass of the symmetric head: pair p is the virtual clouds p (object i queries object j) and p + P (j queries i).
    live = (count, period = P, offset) gates the stage-1 apply, the stage-2 kv and apply and, on the un-pooled route, the
    head, which then writes dead_value itself; None is the un-gated launch of each.  -> logits, whether they are final"""
    kv1, pooled_ok = state
    n_pts, n_pairs = h.shape[2], i.shape[0]
    q_idx = torch.cat([i, j]).contiguous()
    k_idx = torch.cat([j, i]).contiguous()
    s1 = p1.apply(h, None, kv1, n_pts, kv_index=k_idx, q_index=q_idx, n_out=2 * n_pairs, live=live)
    xyz_v = xyz.index_select(0, q_idx.long()).contiguous()
    partner = torch.cat([torch.arange(n_pairs, 2 * n_pairs, device=h.device, dtype=torch.int32),
                         torch.arange(0, n_pairs, device=h.device, dtype=torch.int32)])
    kv2 = p2.kv(s1, xyz_v, live=live)
    if not pooled_ok:
        o = p2.apply(s1, None, kv2, n_pts, kv_index=partner, live=live)
        return model._head(o.device).run(o, live=live, dead_value=dead_value), True
    # round 6: the stage-2 apply launch leaves every virtual cloud's per-channel maximum and sum (512 bytes) instead of
    # its 32 KB output for pool_head to read back; the head then runs over the pooled ROWS on the matrix core
    # (the pooled rows of dead pairs are zeros: the row kernels read every row, and a row's logit depends on that row alone)
    pl = p2.apply(s1, None, kv2, n_pts, kv_index=partner, pooled=True, live=live)         # (2n, 2, C): [max | sum]
    a, b2 = pl[:n_pairs], pl[n_pairs:]
    feat = torch.cat([torch.maximum(a[:, 0], b2[:, 0]), (a[:, 1] + b2[:, 1]) / float(2 * n_pts)], dim=1)
    return model._head_rows(feat), False


def _chunk_one_way(model, p1, p2, h, xyz, state, i, j, live, dead_value):
    """one pass of match_type 'xcorr-baseline' / 'xcorr' (ReIDNet.xcorr_baseline / xcorr): the template of both cross
    stages is object j's original features, so kv1 and kv2 are per OBJECT and pair (i, j) is ONE virtual cloud: object i's
    tokens against object j's state, twice.  live gates the two applies (never given with the local stages, which have no
    gated form).  -> logits, whether they are final"""
    kv1, kv2, local = state
    n_pts, n_pairs = h.shape[2], i.shape[0]
    i, j = i.contiguous(), j.contiguous()
    s = p1.apply(h, None, kv1, n_pts, kv_index=j, q_index=i, n_out=n_pairs, live=live)
    if local:
        xyz_v = xyz.index_select(0, i.long()).contiguous()
        s = model.local_stage1(s, xyz_v)
    # (a dead pair's rows of the gated stage-2 output are zeros: pooling and the head read every row, and a row's
    # logit depends on that row alone)
    buf = None if live is None else torch.zeros((n_pairs, p2.cfinal or p2.cout, n_pts), dtype=torch.float32, device=h.device)
    s = p2.apply(s, None, kv2, n_pts, kv_index=j, live=live, out=buf)
    if local:
        s = model.local_stage2(s, xyz_v)
    return model._head_rows(model.get_pooled_feats(s)), False


def match_pairs(model, h, xyz, pairs, count=None, dead_value=0.0):
    """ReIDNet.match_gallery (its docstring has the contract) for the heads made of the two cross stages: h (M,C,N), xyz
    (M,N,3), pairs (P,2) -> logits (P,).  With count the passes are gated wherever the head has a gated form, and what a
    pass did not settle itself is set to dead_value afterwards."""
    one_way = model.match_type != "xcorr_eff"
    local = model.match_type == "xcorr"
    if local and (model.local_stage1 is None or model.local_stage2 is None):
        raise L.PcrError("match_type='xcorr' needs local_stage1 / local_stage2 (local_self_attention)")
    count = pair_count(count)
    h, xyz = h.contiguous(), xyz.contiguous()
    n_pts = h.shape[2]
    p1 = model.cross_stage1.plan(h.device)
    p2 = model.cross_stage2.plan(h.device)
    gated = count is not None and not local
    if gated and not (p1.live_ok() and p2.live_ok()):
        raise L.PcrError("match_gallery: count= needs matching stages the gated launches cover "
                         "(pcr_attn_live_ok: d_model = 64 with 64-channel features)")
    # the key/value state of the ORIGINAL features: once per object, shared by all its pairs
    if one_way:
        body, state = _chunk_one_way, (p1.kv(h, xyz), p2.kv(h, xyz), local)
    else:
        # (pcr_attn_apply_pool_ok: the launch shape and the arithmetic decide, never the number of pairs)
        body, state = _chunk_symmetric, (p1.kv(h, xyz), p2.pool_ok(n_pts, n_pts))
    out = []
    for lo in range(0, pairs.shape[0], model.GALLERY_CHUNK):
        pc = pairs[lo:lo + model.GALLERY_CHUNK]
        n_pairs = pc.shape[0]
        i = pc[:, 0].to(device=h.device, dtype=torch.int32)
        j = pc[:, 1].to(device=h.device, dtype=torch.int32)
        logits, final = body(model, p1, p2, h, xyz, state, i, j, (count, n_pairs, lo) if gated else None, dead_value)
        if count is not None and not final:
            alive = torch.arange(lo, lo + n_pairs, device=h.device, dtype=torch.int32) < count
            logits = torch.where(alive, logits, logits.new_full((), float(dead_value)))
        out.append(logits)
    if not out:
        return torch.empty(0, dtype=torch.float32, device=h.device)
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)
