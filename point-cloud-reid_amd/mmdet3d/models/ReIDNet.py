"""`ReIDNet`: siamese point-cloud re-identification model with the reference's model-level plugin
API (bentherien/point-cloud-reid, mmdet3d/models/ReIDNet.py:40-96 module_obj/build_module,
:111-776 ReIDNet), so that configs_reid/* build unchanged through FUSIONMODELS / build_model.

What runs where: both clouds of every pair go through the backbone in one batch
(siamese_forward, ref :311-332); the two-stage bidirectional cross-attention (xcorr_eff, ref
:231-247) runs on all 2B clouds at once with a partner index instead of four separate calls;
'point-cat' + pool 'both' + match head (ref :526-534, :444-462) is a single launch.  All of it
is libpcr_hip.so; this file only owns parameters, shapes and the mmdet-style entry points.
"""
import contextlib
import copy
from collections import OrderedDict

import torch
import torch.nn as nn

from pcr_amd import engine, frame, gallery, retrieval
from pcr_amd import _lib as L
from pcr_amd.lazylog import LazyScalars
from .attention import corss_attention, cross_lin_attn, local_self_attention
from .backbone_net import Pointnet_Backbone
from .dgcnn_orig import DGCNN
from .builder import FUSIONMODELS
from .lanegcn_nets import LinearRes
from .pointnet import PointNet
from .pointnet2_ssg import PointNet2SSG


class _OutOfScope(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()
        raise NotImplementedError("%s is outside the siamese point-cloud hot path rebuilt here "
                                  "(SURVEY.md section 8f)" % type(self).__name__)


class PostRes(_OutOfScope):
    pass


# type names a config may use (reference ReIDNet.py:40-75)
module_obj = {
    "Linear": nn.Linear,
    "ReLU": nn.ReLU,
    "LSTM": nn.LSTM,
    "GroupNorm": nn.GroupNorm,
    "Embedding": nn.Embedding,
    "LayerNorm": nn.LayerNorm,
    "PostRes": PostRes,
    "LinearRes": LinearRes,
    "Pointnet_Backbone": Pointnet_Backbone,
    "corss_attention": corss_attention,
    "local_self_attention": local_self_attention,
    "Conv1d": nn.Conv1d,
    "Conv2d": nn.Conv2d,
    "BatchNorm1d": nn.BatchNorm1d,
    "Sigmoid": nn.Sigmoid,
    "cross_lin_attn": cross_lin_attn,
    "dgcnn": DGCNN,
    "PointNet": PointNet,
    # not in the reference table: BASELINE config 2's build-defined PointNet++ SSG encoder
    "PointNet2SSG": PointNet2SSG,
}


def build_module(cfg):
    """None / {} -> None, list -> nn.Sequential, dict -> module_obj[type](**rest).
    Like the reference (:77-96) this consumes the 'type' key of the dict it is given."""
    if cfg is None or cfg == {}:
        return None
    if isinstance(cfg, list):
        return build_sequential(cfg)
    cls_ = module_obj[cfg["type"]]
    del cfg["type"]
    return cls_(**cfg)


def build_sequential(module_list):
    if module_list is None or module_list == {}:
        return None
    return nn.Sequential(*[build_module(cfg) for cfg in module_list])


def get_accuracy(y_true, y_prob):
    assert y_true.ndim == 1 and y_true.size() == y_prob.size()
    y_prob = y_prob > 0.5
    return (y_true == y_prob).sum().item() / y_true.size(0)


@FUSIONMODELS.register_module()
class ReIDNet(nn.Module):
    def __init__(self, hidden_size, backbone, cls_head, match_head, shape_head, fp_head, downsample,
                 cross_stage1, local_stage1, cross_stage2, local_stage2, match_type="xcorr", pool_type="max",
                 combine="cat", compute_summary=True, train_cfg=None, test_cfg=None,
                 backbone_list=[512, 256, 128], use_dgcnn=False,
                 losses_to_use=dict(kl=True, match=True, cls=True, shape=True, fp=True, dense=False),
                 output_sequence_size=32, alpha=dict(kl=1, match=1, cls=1, shape=1, fp=1, triplet=1, dense=1),
                 triplet_sample_num=5, triplet_loss=dict(margin=0.2, p=2), eval_only=False, use_o=False,
                 eval_flip=False, sampling=None):
        super().__init__()
        self.eval_only = eval_only
        self.hidden_size = hidden_size
        self.match_type = match_type
        self.backbone = build_module(backbone)
        self.cls_head = build_module(cls_head)
        self.match_head = build_module(match_head)
        self.shape_head = build_module(shape_head)
        self.fp_head = build_module(fp_head)
        self.downsample = build_module(downsample)
        self.cross_stage1 = build_module(cross_stage1)
        self.local_stage1 = build_module(local_stage1)
        self.cross_stage2 = build_module(cross_stage2)
        self.local_stage2 = build_module(local_stage2)

        self.losses_to_use = dict(kl=False, match=True, cls=False, shape=False, fp=False, dense=False)
        self.losses_to_use.update(losses_to_use)
        self.backbone_list = backbone_list
        self.output_sequence_size = output_sequence_size
        self.pool_type = pool_type
        self.bce = nn.BCEWithLogitsLoss()
        self.alpha = alpha
        self.use_o = use_o
        self.eval_flip = eval_flip
        self.verbose = False
        self.sampling = sampling        # None: pair p is cloud p of each side; 'cartesian': all b x b pairs (forward_train)
        self.compute_summary = compute_summary
        self.use_dgcnn = use_dgcnn
        self.combine = combine
        self.triplet_sample_num = triplet_sample_num
        self.triplet_cfg = dict(triplet_loss or {})
        # the triplet draw's own seed (its device copy advances by one per draw) and, for tests, the words that take the
        # generator's place: (B * triplet_sample_num) int32 on the device (pcr_triplet_draw_i32's rand)
        self.triplet_seed = 0
        self.triplet_rand = None
        self._head_plan = None
        self._head_key = None

    # ------------------------------------------------------------------ inputs
    @staticmethod
    def _stack(*lists):
        return [torch.stack(x, dim=0) for x in lists]

    @staticmethod
    def _cat(*lists):
        return [torch.cat(x, dim=0) for x in lists]

    def preprocess_inputs(self, sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2):
        sparse_1, sparse_2, dense_1, dense_2 = self._stack(sparse_1, sparse_2, dense_1, dense_2)
        label_1, label_2, id_1, id_2 = self._cat(label_1, label_2, id_1, id_2)
        if self.eval_flip:
            return sparse_2, sparse_1, dense_2, dense_1, label_2, label_1, id_2, id_1
        return sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2

    def preprocess_inputs_size(self, sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2,
                               size_1, size_2):
        sparse_1, sparse_2, dense_1, dense_2 = self._stack(sparse_1, sparse_2, dense_1, dense_2)
        return (sparse_1, sparse_2, dense_1, dense_2,
                *self._cat(label_1, label_2, id_1, id_2, size_1, size_2))

    def preprocess_inputs_size_vis(self, sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2,
                                   size_1, size_2, vis_1, vis_2):
        sparse_1, sparse_2, dense_1, dense_2 = self._stack(sparse_1, sparse_2, dense_1, dense_2)
        return (sparse_1, sparse_2, dense_1, dense_2,
                *self._cat(label_1, label_2, id_1, id_2, size_1, size_2, vis_1, vis_2))

    # ------------------------------------------------------------------ split-bf16 guard (pcr_amd/engine.py)
    def _weights_key(self, full=True):
        """identity + version of every parameter and buffer.  full: one walk over the module tree (~150 us for the ~230
        tensors of a ReID model; every guard tick and guard_state() do it), so that REPLACED Parameters
        (load_state_dict(assign=True), m.weight = nn.Parameter(..), re-registered buffers) are seen, not only in-place
        writes; not full: the versions of the tensors found by the last walk (~25 us; precision_level(), several times
        per pass between two ticks)"""
        ts = None if full else self.__dict__.get("_pcr_tensors")
        if ts is None:
            tensors, h, stack = [], 0, [self]
            while stack:
                mod = stack.pop()
                for d in (mod._parameters, mod._buffers):
                    for t in d.values():
                        if t is not None:
                            tensors.append(t)
                            h = ((h * 1000003) ^ id(t)) & 0xFFFFFFFFFFFFFFFF
                for c in mod._modules.values():
                    if c is not None:
                        stack.append(c)
            ts = (tensors, h)
            self.__dict__["_pcr_tensors"] = ts
        v = 0
        for t in ts[0]:
            v += t._version
        return (v, ts[1], len(ts[0]))

    def _guard_active(self):
        return engine.GUARD and engine.PRECISION == "bf16x3" and not self.training

    def precision_level(self):
        """guard level of these weights: the calibrated one (0 before calibration -- every inference entry point
        calibrates on its first batch, _guard_tick / _match_level, so an uncalibrated 0 is only seen inside a HIP-graph
        capture or on host tensors; always 0 in training mode, with the guard off, or outside "bf16x3" mode)"""
        if not self._guard_active():
            return 0
        st = self.__dict__.get("_pcr_guard")
        return st["level"] if st is not None and st["key"] == self._weights_key(full=False) else 0

    def guard_state(self):
        """what calibrate_precision (and the sentinel since) measured for the current weights, or None"""
        st = self.__dict__.get("_pcr_guard")
        if st is None or st["key"] != self._weights_key():
            return None
        return {k: v for k, v in st.items() if k != "key"}

    _INHERIT = contextlib.nullcontext()

    @staticmethod
    def _at_level(lvl):
        """with self._at_level(self.precision_level() / self._match_level(..)): the launches inside run at this model's guard
        level.  Level 0 INHERITS the surrounding level instead of setting 0: calibrate_precision and _sentinel call the hot
        path inside a guard_level of their own"""
        return engine.guard_level(lvl) if lvl else ReIDNet._INHERIT

    def _hot(self, s1, s2):
        xyz1, xyz2, h1, h2 = self._siamese_forward(s1, s2)
        return self._match_logits(h1, h2, xyz1, xyz2, inference=True)[0]

    def calibrate_precision(self, sparse_1, sparse_2, bound=None, max_pairs=64):
        """split-bf16 guard: run the hot path on (up to max_pairs of) this batch in f32 and at guard levels 0, 1, 2, keep the
        first level whose logits stay within engine.GUARD_ACCEPT x `bound` (engine.GUARD_BOUND, half the 1e-4 parity bound) of the f32 path's,
        for as long as the weights do not change (the sentinel re-checks it on live batches: _guard_tick).
        -> {"level", "dlogit": {level: max |logit - f32 logit|}, ...}"""
        bound = engine.GUARD_BOUND if bound is None else float(bound)
        s1, s2 = sparse_1[:max_pairs].contiguous(), sparse_2[:max_pairs].contiguous()
        self.__dict__.pop("_pcr_guard", None)
        dl, level = {}, 0
        if engine.PRECISION == "bf16x3" and not self.training:
            self.__dict__["_pcr_guard_busy"] = True
            prof, engine.PROFILE = engine.PROFILE, None          # (the guard's own passes are not part of a profiled pass)
            try:
                with torch.no_grad():
                    with engine.precision("f32"):
                        ref = self._hot(s1, s2)
                    for level in (0, 1, 2):
                        with engine.guard_level(level):
                            dl[level] = float((self._hot(s1, s2) - ref).abs().max())
                        if dl[level] <= bound * engine.GUARD_ACCEPT:      # (a margin for the next batch: engine.GUARD_ACCEPT)
                            break
            finally:
                self.__dict__["_pcr_guard_busy"] = False
                engine.PROFILE = prof
        st = dict(key=self._weights_key(), level=level, dlogit=dl, bound=bound, pairs=int(s1.shape[0]), calls=0,
                  sentinel=dict(every=engine.GUARD_EVERY, checks=0, worst=0.0, raised=[]))
        self.__dict__["_pcr_guard"] = st
        return self.guard_state()

    def _sentinel(self, c1, c2, st):
        """run-time re-check of the calibrated level on (up to engine.GUARD_SENTINEL_PAIRS of) the LIVE batch: the f32 path
        against the current level; on a breach of the bound the level of this weight version is raised to the first
        one that holds (2 = the f32 path always does) BEFORE the batch itself is computed, and the event is logged.
        The sampled pairs rotate through the batch from check to check."""
        sen = st["sentinel"]
        m = min(engine.GUARD_SENTINEL_PAIRS, int(c1.shape[0]))
        lo = (sen["checks"] * m) % max(1, int(c1.shape[0]) - m + 1)
        s1, s2 = c1[lo:lo + m].contiguous(), c2[lo:lo + m].contiguous()
        self.__dict__["_pcr_guard_busy"] = True
        prof, engine.PROFILE = engine.PROFILE, None
        try:
            with torch.no_grad():
                with engine.precision("f32"):
                    ref = self._hot(s1, s2)
                level = st["level"]
                while True:
                    with engine.guard_level(level):
                        d = float((self._hot(s1, s2) - ref).abs().max()) if level < 2 else 0.0
                    if d <= st["bound"] or level >= 2:
                        break
                    level += 1
        finally:
            self.__dict__["_pcr_guard_busy"] = False
            engine.PROFILE = prof
        sen["checks"] += 1
        if level != st["level"]:
            import logging
            logging.getLogger("pcr_amd.guard").warning(
                "split-bf16 guard: live batch %d deviates from the f32 path beyond %.1e at level %d; these weights run "
                "at level %d from here on", st["calls"], st["bound"], st["level"], level)
            sen["raised"].append(dict(call=st["calls"], was=st["level"], now=level))
            st["level"] = level
        else:
            sen["worst"] = max(sen["worst"], d)

    def _guard_tick(self, c1, c2):
        """top of every inference entry point that sees raw clouds (c1, c2: (B,N,3) halves of pairs, or the two halves of a
        gallery): lazy calibration on the first batch of a weight version (the tracker entry points ran
        unguarded until someone called calibrate_precision by hand), then the sentinel every engine.GUARD_EVERY batches.
        Inside a HIP-graph capture nothing can be measured (host reads): the captured launches keep the level the model
        has -- calibrate before capturing, as bench.py does."""
        if not self._guard_active() or self.__dict__.get("_pcr_guard_busy") or not c1.is_cuda or c1.shape[0] == 0:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        st = self.__dict__.get("_pcr_guard")
        if st is None or st["key"] != self._weights_key():
            self.calibrate_precision(c1, c2)
            return
        st["calls"] += 1
        every = engine.GUARD_EVERY
        if every > 0 and st["level"] < 2 and st["calls"] % every == 0:
            self._sentinel(c1, c2, st)

    @staticmethod
    def _halves(pts):
        """a batch of single clouds (forward_inference) as pairs for the guard: first half against second half"""
        m = pts.shape[0] // 2
        return (pts[:m], pts[m:2 * m]) if m else (pts, pts)

    def _raw_clouds(self, xyz1, xyz2):
        """match-only entry (features computed elsewhere): the raw clouds are what the point-major backbones return as
        xyz; PointNet / DGCNN hand back a transformed, channel-major xyz that cannot be re-encoded"""
        if self.use_dgcnn or isinstance(self.backbone, PointNet):
            return None
        return xyz1, xyz2

    # ------------------------------------------------------------------ encoder
    def forward_inference(self, pts_batched):
        # (PointNet / DGCNN take channel-major clouds (B,3,N); the guard's pairs are point-major like siamese_forward's)
        cm = self.use_dgcnn or isinstance(self.backbone, PointNet)
        self._guard_tick(*self._halves(pts_batched.permute(0, 2, 1) if cm else pts_batched))
        with torch.no_grad(), self._at_level(self.precision_level()):
            return self.backbone(pts_batched, self.backbone_list)

    def forward_inference_boxes(self, points, boxes, n=None, **crop_args):
        """a sweep (P, C >= 3) and boxes (M, 7) on the device -> (xyz, feats, lengths): pcr_amd.crops.crops_from_boxes (the
        reference tracker's interpolate_per_frame + get_input_batch, trackers/deprecated/pc_utils.py:31-96) followed by
        forward_inference.  n defaults to the encoder's input size, backbone_list[0], for the Point-Transformer backbone
        and must be given for the others.  A box without points is encoded as a cloud of zeros, as in the reference;
        masking it is the caller's decision (lengths == 0; tracking_point_reid.py:93-100)."""
        from pcr_amd import crops
        if n is None:
            if not isinstance(self.backbone, Pointnet_Backbone):
                raise ValueError("forward_inference_boxes: n (points per crop) must be given for this backbone")
            n = int(self.backbone_list[0])
        if crop_args.get("return_frames"):
            raise ValueError("forward_inference_boxes returns (xyz, feats, lengths); ask crops_from_boxes for frames")
        clouds, lengths = crops.crops_from_boxes(points, boxes, n, **crop_args)
        if self.use_dgcnn or isinstance(self.backbone, PointNet):
            clouds = clouds.permute(0, 2, 1).contiguous()
        xyz, feats = self.forward_inference(clouds)
        return xyz, feats, lengths

    def siamese_forward(self, sparse_1, sparse_2):
        self._guard_tick(sparse_1, sparse_2)
        with self._at_level(self.precision_level()):
            return self._siamese_forward(sparse_1, sparse_2)

    def _siamese_forward(self, sparse_1, sparse_2):
        """(B,N,3) x 2 -> xyz1, xyz2 (B,N,3), h1, h2 (B,C,N); one backbone pass over 2B clouds"""
        assert sparse_1.shape == sparse_2.shape
        b, num_points, _ = sparse_1.shape
        both = torch.cat([sparse_1, sparse_2], dim=0)
        if self.use_dgcnn or isinstance(self.backbone, PointNet):
            # per-point 1024-d encoder features, reduced per point by `downsample` (ref :316-324)
            xyz, h = self.backbone(both.permute(0, 2, 1).contiguous(), self.backbone_list)
            if self.downsample is not None:
                if self.training:
                    from pcr_amd import train_graph
                    h = train_graph.downsample_points(self.downsample, h)
                else:
                    from pcr_amd import rows
                    h = rows.downsample_points(self.downsample, h)
            xyz = xyz.permute(0, 2, 1)
            return xyz[:b], xyz[b:], h[:b], h[b:]
        xyz, h = self.backbone(both, self.backbone_list)
        return xyz[:b], xyz[b:], h[:b], h[b:]

    # ------------------------------------------------------------------ matching
    @staticmethod
    def _pair_batch(a1, a2):
        """two halves -> one (2B, ...) tensor, without a copy when they already are adjacent views"""
        if (a1.is_contiguous() and a2.is_contiguous() and a1.untyped_storage().data_ptr() == a2.untyped_storage().data_ptr()
                and a2.storage_offset() == a1.storage_offset() + a1.numel()):
            return a1.as_strided((2 * a1.shape[0],) + tuple(a1.shape[1:]), a1.stride(), a1.storage_offset())
        return torch.cat([a1, a2], dim=0)

    def _xcorr_eff_batched(self, h1, xyz1, h2, xyz2):
        b = h1.shape[0]
        feats = self._pair_batch(h1, h2).contiguous()
        xyz = self._pair_batch(xyz1, xyz2).contiguous()
        # (built on the device: a pageable host-to-device copy here stalls the stream -- measured on the gallery path,
        # where the same 256 KB index copy cost 45 ms every third step)
        partner = torch.cat([torch.arange(b, 2 * b, device=feats.device, dtype=torch.int32),
                             torch.arange(0, b, device=feats.device, dtype=torch.int32)])
        s1 = self.cross_stage1.forward_paired(feats, xyz, partner)
        return self.cross_stage2.forward_paired(s1, xyz, partner)     # (2B,C,N): [o1; o2]

    def xcorr_eff(self, o1, xyz1, o2, xyz2, combine="add"):
        b = o1.shape[0]
        o = self._xcorr_eff_batched(o1, xyz1, o2, xyz2)
        o1, o2 = o[:b], o[b:]
        if self.combine == "add":
            out = o1 + o2
        elif self.combine == "minus":
            out = o1 - o2
        elif self.combine == "cat":
            out = torch.cat([o1, o2], dim=1)
        elif self.combine == "point-cat":
            out = torch.cat([o1, o2], dim=2)
        else:
            raise NotImplementedError(self.combine)
        return out, o1, o2

    def _head(self, device):
        if not (isinstance(self.match_head, nn.Sequential) and len(self.match_head) == 2
                and isinstance(self.match_head[0], LinearRes) and isinstance(self.match_head[1], nn.Linear)):
            raise L.PcrError("fused match head expects [LinearRes, Linear] as in every ReID config")
        key = (str(device), engine.param_version(self.match_head))
        if self._head_key != key:
            self._head_plan = engine.HeadPlan(self.match_head[0], self.match_head[1], device)
            self._head_key = key
        return self._head_plan

    def get_pooled_feats(self, h_cat):
        from pcr_amd import rows
        if self.pool_type == "max":
            # nn.MaxPool1d(output_sequence_size) on the permuted (B,N,C) tensor: a max over channel windows (reference
            # :145, :526-528) -- (B,N) when C == output_sequence_size, as in reid_pts_point-transformer_baseline.py
            return rows.pool_channel_max(h_cat, self.output_sequence_size)
        if self.pool_type == "both":
            return rows.pool_both(h_cat)
        raise NotImplementedError("pool_type=%r" % self.pool_type)

    def _fused_matching(self):
        return self.match_type == "xcorr_eff" and self.combine == "point-cat" and self.pool_type == "both"

    def _head_rows(self, pooled):
        """match_head ([LinearRes..., Linear]) on pooled rows (B,F) through the row kernels (pcr_amd/rows.py)"""
        from pcr_amd import rows
        x = pooled.t().contiguous().unsqueeze(0)                 # (1,F,B): channel-major, samples as tokens
        return rows.downsample_points(self.match_head, x).reshape(-1)

    def xcorr(self, search_feat, search_xyz, template_feat, template_xyz):
        """cross -> local -> cross -> local on the search branch (reference ReIDNet.py:250-256)"""
        a = self.cross_stage1(search_feat, search_xyz, template_feat, template_xyz)
        b = self.local_stage1(a, search_xyz)
        c = self.cross_stage2(b, search_xyz, template_feat, template_xyz)
        return self.local_stage2(c, search_xyz)

    def xcorr_baseline(self, search_feat, search_xyz, template_feat, template_xyz):
        a = self.cross_stage1(search_feat, search_xyz, template_feat, template_xyz)
        return self.cross_stage2(a, search_xyz, template_feat, template_xyz)

    def _match_logits(self, h1, h2, xyz1, xyz2, inference=False):
        """logits (B) and the stage-2 features; fused single-launch tail for the configuration every point
        ReID config uses, generic composition (reference ReIDNet.py:387-462) for the other variants"""
        if self.training:
            # training mode: the differentiable HIP graph (raises PcrError for the matchings it does not cover -- the
            # inference compositions below have no backward)
            from pcr_amd import train_graph
            return train_graph.match_logits(self, h1, xyz1, h2, xyz2)
        if self._fused_matching():
            o = self._xcorr_eff_batched(h1, xyz1, h2, xyz2)
            return self._head(o.device).run(o), o
        if self.match_type == "xcorr_eff":
            match_in, o1, o2 = self.xcorr_eff(h1, xyz1, h2, xyz2, self.combine)
            return self._head_rows(self.get_pooled_feats(match_in)), torch.cat([o1, o2], dim=0)
        if self.match_type == "xcorr":
            if self.local_stage1 is None or self.local_stage2 is None:
                raise L.PcrError("match_type='xcorr' needs local_stage1 / local_stage2 (local_self_attention)")
            match_in = self.xcorr(h1, xyz1, h2, xyz2)
            return self._head_rows(self.get_pooled_feats(match_in)), None
        if self.match_type == "xcorr-baseline":
            match_in = self.xcorr_baseline(h1, xyz1, h2, xyz2)
            return self._head_rows(self.get_pooled_feats(match_in)), None
        if self.match_type == "concat":
            if inference:     # the reference's inference entry point pools with self.maxpool whatever pool_type (:455-457)
                from pcr_amd import rows
                pool = lambda h: rows.pool_channel_max(h, self.output_sequence_size)
            else:
                pool = self.get_pooled_feats
            cat = torch.cat([pool(h1), pool(h2)], dim=1)
            return self._head_rows(cat), None
        raise NotImplementedError("match_type=%r" % self.match_type)

    def _match_level(self, xyz1, xyz2):
        """level for an entry point that only sees features: the calibrated one; an uncalibrated weight version is
        calibrated from the raw clouds (xyz of the point-major backbones) or, where they cannot be recovered, runs the
        matching in f32 (level 2) -- never unguarded"""
        if not self._guard_active() or self.__dict__.get("_pcr_guard_busy"):
            return self.precision_level()
        st = self.__dict__.get("_pcr_guard")
        if st is not None and st["key"] == self._weights_key(full=False):
            return st["level"]
        if self.guard_state() is None and xyz1.is_cuda and not torch.cuda.is_current_stream_capturing():
            raw = self._raw_clouds(xyz1, xyz2)
            if raw is None or raw[0].shape[0] == 0:
                return 2
            self.calibrate_precision(*raw)
        return self.precision_level()

    def match_forward_inference(self, h1, h2, xyz1, xyz2):
        with self._at_level(self._match_level(xyz1, xyz2)):
            return self._match_logits(h1, h2, xyz1, xyz2, inference=True)[0]

    # the launches index clouds by a 16-bit grid dimension: at most 32 k pairs (64 k virtual clouds) per pass of match_gallery
    GALLERY_CHUNK = 32000

    def match_gallery(self, h, xyz, pairs, count=None, dead_value=0.0):
        """Amortised matching (the reference's tracker use-case of forward_inference +
        match_forward_inference, ReIDNet.py:189-191, 444-462): every object is encoded ONCE, then any list
        of (i, j) combinations is scored.  h (M,C,N), xyz (M,N,3) from forward_inference / siamese_forward;
        pairs (P,2) integer tensor -> logits (P), identical to match_forward_inference(h[i], h[j], ...).
        Stage-1 key/value state is computed once per object and shared by all its pairs.
        count ((1,) int32 device tensor; None: every pair): only pairs[:count] are real, as in the fixed-shape list of
        compare_pairs.  The pair launches read the count themselves and do no work for the rest (engine.AttnPlan live=:
        nothing of a pair beyond count is read, its indices included); logits[:count] are bit for bit those of the un-gated
        call, logits[count:] are dead_value exactly.  No host read: a captured graph follows the count from replay to
        replay.

        Heads.  xcorr_eff / point-cat / both (symmetric: both directions of a pair are evaluated), and the three one-way
        heads of the reference's baseline configs, for which pair (i, j) is NOT pair (j, i) -- i is the search side, the
        first argument of match_forward_inference:
          concat          the embedding head (embed / match_embeddings): pooled once per object, one launch for the list;
                          count= gates that launch.
          xcorr-baseline  both cross stages take the template's ORIGINAL features, so the key/value state of both stages
                          is per object and a pair is one virtual cloud; count= gates the two applies.
          xcorr           as xcorr-baseline with the local stages in between.  The local stages have no gated form: with
                          count= the whole list is scored (the padding (0, 0) of compare_pairs is a valid pair) and the
                          logits beyond count are replaced by dead_value -- this head saves no work for padding."""
        with self._at_level(self._match_level(*self._halves(xyz))):
            if self.match_type == "concat":
                return self.match_embeddings(self.embed(h), pairs, count=count, dead_value=dead_value)
            if self.match_type in ("xcorr", "xcorr-baseline") or self._fused_matching():
                return gallery.match_pairs(self, h, xyz, pairs, count, dead_value)
            raise NotImplementedError("match_gallery covers the xcorr_eff / point-cat / both matching head and the concat, "
                                      "xcorr-baseline and xcorr heads")

    def match_gallery_train(self, h, xyz, pairs, count=None):
        """The differentiable twin of match_gallery, for training on a pair list (include/pcr.h section C3; INTEGRATION.md
        "training on a pair list"): h (M,C,N), xyz (M,N,3) are the objects of THIS step as the training-mode encoder
        returned them (siamese_forward; h carries its autograd history), pairs (cap,2) int32 on the device, count a (1,)
        int32 device tensor or None = cap -> logits (cap,).  Slot p scores as the training graph scores the one pair
        (h[i], h[j]), i first; a dead slot (p >= count, or an index outside [0, M)) has logit 0.0 and sends exactly zero to
        every gradient.  Objects are encoded once however many slots name them; their gradients are summed in list order
        (pcr_index_sum_f32: no float atomics, bit-reproducible).  No host read: Trainer(graph=True) captures it.
        pcr_amd.train_graph.list_loss forms the masked loss.  Training mode only -- match_gallery is the inference form."""
        if not self.training:
            raise L.PcrError("match_gallery_train: the model is in eval mode; match_gallery is the inference form")
        from pcr_amd import train_graph
        return train_graph.match_logits_list(self, h, xyz, pairs, count)[0]

    def embed(self, h):
        """h (M,C,N) from forward_inference -> (M,F) embeddings of the 'concat' head, F = N: what the inference entry point
        pools each side with (self.maxpool whatever pool_type, reference ReIDNet.py:455-457) -- 4 F bytes per object to
        store instead of the (C,N) features.  C > output_sequence_size (a 3-D pool) is refused."""
        from pcr_amd import rows
        if self.match_type != "concat":
            raise L.PcrError("embed: the embedding form is the match_type='concat' head (got %r)" % self.match_type)
        L.require_cuda(h)
        if h.dim() != 3 or h.shape[1] > self.output_sequence_size:
            raise L.PcrError("embed: features (M, C, N) with C <= output_sequence_size = %d expected, got %s"
                             % (self.output_sequence_size, tuple(h.shape)))
        return rows.pool_channel_max(h, self.output_sequence_size)

    def match_embeddings(self, emb, pairs, count=None, dead_value=0.0):
        """emb (M,F) from embed, pairs (P,2) -> logits (P): pair (i, j) scores as match_forward_inference(h[i:i+1],
        h[j:j+1], ...) does (i first: the head is not symmetric).  The per-object tables of the head's first layer are made
        once, the rest is one launch over the whole list (pcr_amd/pairs_head.py), f32 arithmetic in every precision mode.
        count / dead_value as in match_gallery: pairs[count:] are neither read nor scored.  A pair with an index outside
        [0, M) gets NaN."""
        from pcr_amd import pairs_head
        if self.match_type != "concat":
            raise L.PcrError("match_embeddings: the embedding form is the match_type='concat' head (got %r)" % self.match_type)
        L.require_cuda(emb)
        pl = pairs_head.plan(self.match_head, emb.device)
        u, v = pairs_head.tables(pl, emb)
        return pairs_head.pair_logits(pl, emb, u, v, pairs, count=gallery.pair_count(count), dead_value=dead_value)

    def associate(self, track_feats, track_xyz, track_labels, track_lengths, det_feats, det_xyz, det_labels, det_lengths,
                  min_points=2, num_classes=8, cap=None, live_only=False, decisions=None, by_class=False, **cost_args):
        """One frame of the reference tracker's association on the device (pcr_amd/associate.py): the class-gated pair
        list (get_labels_to_compare, tracking_point_reid.py:15-33), match_gallery over [tracks | detections], the
        augmented cost matrix (get_cost_mat_margin, tracking_association.py:22-53) and the linear assignment the
        reference hands to scipy (:141) -- no host read anywhere.  track_feats (T,C,N) / track_xyz (T,N,3) are the
        caller's stored track features, det_* what forward_inference returned for this frame's crops; lengths may be
        None (no length filter); cost_args go to association_cost (track_miss, det_new, dist, dist_max, dist_penalty,
        fill).  live_only: match_gallery scores the count real pairs of the list only (count=; logits[count:] are then 0.0
        instead of the padding pairs' scores -- association_cost reads logits[:count], so everything else is bit-identical).
        -> dict(track_to_det (T,), det_to_track (D,) [-1 = none], pairs, count, logits, cost, info).
        by_class: the assignment is solved class by class, one wave per class, instead of as one problem (pcr.h, "the
        block rule"; INTEGRATION.md 2c: the matrix is block-diagonal because compare_pairs lists pairs of one class only).
        Everything returned is the same bits -- decode_info[1] alone may be smaller, no leftovers being paired across
        classes -- info stays one word (the maximum over the blocks) and the dict gains block_info (num_classes + 1,).

        decisions=dict(detection=(names...), tracking=(names...), det_values=(dd, D) or None, track_values=(td, T) or None,
        kind="margin" | "softmax", reduce=False) runs the reference's tracker with any set of decisions:
        association_cost_multi builds the (T + dd*D, D + td*T) matrix (cost_args: dist, dist_max, dist_penalty, fill; no
        dist with the softmax kind), decode_assignment turns the assignment into decisions, and the dict gains det_decision
        (D,), track_decision (T,) [0 = matched, 1 + k = decision k of the SORTED names, 1 + dd / 1 + td = unmatched], born
        (D,) = the detections that took 'det_newborn', kill (T,) = the tracks that took 'track_false_positive' (all zero when
        the name is absent) and decode_info (4,).  An empty side is no special case then: the detections of a first frame
        still take their decisions."""
        return frame.associate(self, track_feats, track_xyz, track_labels, track_lengths, det_feats, det_xyz, det_labels,
                               det_lengths, min_points, num_classes, cap, live_only, decisions, by_class, cost_args)

    def retrieve(self, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths, query_ids=None,
                 gallery_ids=None, topk=10, exclude=None, min_points=2, num_classes=8, live_only=False):
        """Rank a gallery for every query on the device (pcr_amd/retrieval.py; INTEGRATION.md "2h. Ranking a gallery"):
        compare_pairs with the queries in the tracks' place (a pair of one class, both sides of at least min_points points
        when lengths are given), match_gallery over [queries | gallery], score_matrix (-inf where no pair was listed) and
        rank_gallery -- no host read beyond the guard's first-batch calibration that every inference entry point has.
        q_feats (Q,C,N) / q_xyz (Q,N,3) and g_feats (G,C,N) / g_xyz (G,N,3) are what forward_inference returned;
        query_ids (Q,) / gallery_ids (G,) int32 name identities (< 0, or None: none -- then only topk_* and n_cand mean
        anything); exclude (Q,) int32 names the one gallery entry a query skips (its own observation in a gallery that
        holds the queries).  live_only: match_gallery scores the count listed pairs only.
        -> rank_gallery's dict (topk_idx, topk_score (Q, topk), n_cand, n_true, first_hit, ap, info (Q,)) plus pairs,
        count, logits and scores (Q, G)."""
        return retrieval.retrieve(self, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths, query_ids,
                                  gallery_ids, topk, exclude, min_points, num_classes, live_only)

    def retrieve_wide(self, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths, query_ids=None,
                      gallery_ids=None, topk=10, exclude=None, min_points=2, num_classes=8, live_only=False,
                      gallery_block=4096, scores=None):
        """`retrieve` for a gallery of up to pcr_amd.retrieval.WIDE_MAX_GALLERY entries (INTEGRATION.md "2h. Ranking a
        gallery"; include/pcr.h section A12).  The gallery is walked in blocks of gallery_block entries (1 to 4096; block b
        covers the columns [b * gallery_block, min(G, (b + 1) * gallery_block))): fill_scores once, then per block
        compare_pairs of the queries against the block's labels and lengths, match_gallery over [queries | the block's
        rows] (the block's count when live_only) and scatter_scores into the block's column window; rank_gallery_wide over
        the whole matrix at the end.  The arguments are retrieve's; exclude and the ids are global gallery indices; scores =
        a (Q, G) float32 buffer to write into.  The per-block pair lists and logits are not kept.
        -> rank_gallery's seven outputs plus scores (Q, G) and counts (blocks,) int32, the blocks' pair counts on the device.
        The number of launches depends on the shapes alone.  For G <= 4096 scores and the seven outputs equal retrieve's bit
        for bit whatever gallery_block is: the logit of a pair does not depend on what else is in its batch."""
        return retrieval.retrieve_wide(self, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths,
                                       query_ids, gallery_ids, topk, exclude, min_points, num_classes, live_only,
                                       gallery_block, scores)

    def track_step(self, bank, sweep, boxes, labels, scores, carry=None, carry_inv=None, min_points=2, num_classes=8,
                   cap=None, n=None, crop_args=None, born=None, kill=None, frame_limit=10, replace_all=False,
                   reset_on_match=False, propagate=True, suppress_threshold=0.15, live_only=False, truth=None,
                   force_truth=False, decisions=None, by_class=False, update_config=None, log=None, **cost_args):
        """One whole tracker frame on the device without a host read (pcr_amd/tracks.py; INTEGRATION.md "2e. Track
        state"; the split-bf16 guard calibrates on the first batch of a weight version, as in every inference entry
        point: run a frame eagerly before capturing): the sweep (P, C >= 3) and this frame's boxes (M <= bank.max_dets, bank.box_width) with labels and
        scores (M,) -> crops and features (forward_inference_boxes, written behind the bank's rows of the gallery), the
        distance prior (bank.distances with carry_inv, current frame -> previous), compare_pairs, match_gallery over
        the bank's gallery, association_cost(dist=...), linear_assignment, bank.update (births, deaths, feature
        replacement, propagation by carry, previous frame -> current; born / kill are the learned decisions' masks) and
        bank.suppress (suppress_threshold None = no track NMS).  The detections are padded to bank.max_dets with label
        -1, which joins nothing.  crop_args go to crops_from_boxes, cost_args to association_cost (track_miss, det_new,
        dist_max, dist_penalty, fill).  live_only: as in associate -- the match runs over the frame's real pairs instead of
        capacity x max_dets of them.  -> associate's dict (track_to_det (capacity,), det_to_track (max_dets,), pairs,
        count, logits, cost, info) plus det_slot, det_id (max_dets,), bank_info (1,) = the newborns dropped for want of
        a free slot, dist, lengths.

        truth = dict(book= a pcr_amd.truth.TruthBook over this bank, boxes= (G <= book.max_gt, bank.box_width), labels=, ids=,
        tte= (G,)) scores the frame against ground-truth tracks (INTEGRATION.md "2g. Ground truth"): book.match and
        book.decide run between the assignment and bank.update, book.record after bank.suppress, and the dict gains det_gt,
        true_det_to_track, det_truth (max_dets,), true_track_to_det, track_truth (capacity,).  force_truth: the true
        association drives bank.update in place of the tracker's own, det_truth == 1 as born and track_truth == 2 as
        kill (the reference's teacher forcing in mode 'gt': the upper bound a matching head is compared against), and
        the book's decision counters score those applied decisions; the returned track_to_det / det_to_track stay the
        tracker's own.  Without truth= nothing new is launched.  truth["identity"] = a pcr_amd.identity.IdentityBook made over
        truth["book"] keeps the identity metrics (INTEGRATION.md "2i. Identity metrics"): its record runs right after
        book.record, one launch; nothing else in the frame changes, and without the key nothing new is launched.

        decisions= (as in associate; det_values may be (dd, M) and is zero-padded to max_dets) runs the frame with any set of
        decisions: the matrix is association_cost_multi's (the margin kind takes dist, the softmax kind does not), the
        decoded born / kill masks -- 'det_newborn' and 'track_false_positive', nothing is born or killed when the name is
        absent, as in the reference, whose updater makes tracks from decision lists only -- drive bank.update, and the dict
        gains det_decision, track_decision, born, kill and decode_info.  born= / kill= cannot be passed with it.  truth= /
        force_truth= work on top unchanged.  Without update_config, propagate stays the bank's one flag for every missed track.

        update_config= (needs decisions=; the reference's dict: match, det_newborn, det_false_positive,
        track_false_positive, track_false_negative, each dict(output=, active=, decom=)) runs the updater as the reference
        configures it (pcr_amd.tracks.UpdateRules): bank.update_rules on the decoded det_decision /
        track_decision takes bank.update's place -- a track that took track_false_negative is propagated, an unmatched one
        waits -- and the dict gains the frame's output table out_valid, out_ids, out_labels, out_scores, out_boxes,
        out_flags (capacity + max_dets rows, the bank's own); bank_info becomes (2,): the dropped newborns and the valid
        rows.  It cannot be combined with born= / kill=, propagate=False or force_truth.  log= a pcr_amd.tracks.SceneLog
        of capacity + max_dets rows per frame: the table is appended after the update and before bank.suppress, as the
        reference forms its output before the track NMS.  truth= and identity= keep working; book.decide still gets the
        decoded born / kill.  Without both arguments nothing new is launched.

        by_class: as in associate -- the assignment runs class by class over block ids made from the bank's and the frame's
        labels on the device each frame (free slots and padded detections share the rest block), so one captured graph
        follows changing classes; the dict gains block_info (num_classes + 1,).  It composes with live_only, decisions=
        and truth=."""
        return frame.track_step(self, bank, sweep, boxes, labels, scores, carry, carry_inv, min_points, num_classes, cap, n,
                                crop_args, born, kill, frame_limit, replace_all, reset_on_match, propagate,
                                suppress_threshold, live_only, truth, force_truth, decisions, by_class, update_config, log,
                                cost_args)

    def get_match_supervision(self, h1, h2, xyz1, xyz2, id_1, id_2):
        return h1, h2, xyz1, xyz2, (id_1 == id_2).float()

    def match_forward(self, h1, h2, xyz1, xyz2, match, log_vars, device, prefix=""):
        if not self.losses_to_use["match"]:
            return None, torch.tensor(0.0, requires_grad=True, device=device), (None, None)
        b = h1.shape[0]
        with self._at_level(self.precision_level()):
            match_preds, o = self._match_logits(h1, h2, xyz1, xyz2)
        match_loss = self.bce(match_preds, match) * self.alpha["match"]
        if o is None:
            o = [None] * (2 * b)
        self._log_match(match_preds, match, match_loss, log_vars, prefix)
        return match_preds, match_loss, (o[:b], o[b:])

    def match_forward_cartesian(self, h1, h2, xyz1, xyz2, id_1, id_2, log_vars, device, prefix=""):
        """match_forward under sampling == 'cartesian' (the reference's rule, ReIDNet.py:339-344): all b x b combinations of
        the two sides, slot i b + j = object i of side 1 against object j of side 2, match = (id_1[i] == id_2[j]), the BCE
        mean over the b^2 slots.  The 2b clouds are encoded once; the list is matched by train_graph.match_logits_list."""
        if not self.losses_to_use["match"]:
            return None, torch.tensor(0.0, requires_grad=True, device=device), (None, None)
        from pcr_amd import train_graph
        b = h1.shape[0]
        pairs = train_graph.cartesian_pairs(b, h1.device)
        match = (id_1[pairs[:, 0].long()] == id_2[(pairs[:, 1] - b).long()]).float()
        match_preds, _ = train_graph.match_logits_list(self, train_graph._joined(h1, h2), train_graph._joined(xyz1, xyz2),
                                                       pairs)
        match_loss = self.bce(match_preds, match) * self.alpha["match"]
        self._log_match(match_preds, match, match_loss, log_vars, prefix)
        return match_preds, match_loss, (None, None)

    def _log_match(self, match_preds, match, match_loss, log_vars, prefix):
        if self.compute_summary and log_vars is not None:
            # the reference's six log entries (ReIDNet.py:426-435: `.item()` each), computed on the device as ONE small
            # tensor and read lazily (pcr_amd/lazylog.py): same keys -- including the reference's swapped
            # num_preds / num_gt naming -- and same values, no host round trip inside the step
            pred = match_preds.detach() > 0                      # sigmoid(x) > 0.5
            m = match.detach()
            n = float(m.numel())
            gt1, p1 = m.sum(), pred.float().sum()
            stats = torch.stack([match_loss.detach().reshape(()), pred.float().eq(m).float().mean(),
                                 n - gt1, gt1, n - p1, p1])
            names = [prefix + k for k in ("match_loss", "match_acc", "num_preds_0", "num_preds_1", "num_gt_0", "num_gt_1")]
            ints = [False, False, True, True, True, True]
            if isinstance(log_vars, LazyScalars):
                log_vars.add_device(names, stats, ints)
            else:
                for k, i, v in zip(names, ints, stats.tolist()):
                    log_vars[k] = int(round(v)) if i else v

    def _check_losses(self):
        # match, cls, fp, kl and triplet run (pcr_amd/train_graph.py aux_losses); shape (chamfer distance over dense
        # clouds, a Conv1d / BatchNorm1d head) and dense (a second encoder pass) have no HIP form
        for k in ("shape", "dense"):
            if self.losses_to_use.get(k, False):
                raise NotImplementedError("loss '%s' is not part of the siamese matching hot path; the ReID configs "
                                          "train with match, cls, fp, kl and triplet at most (SURVEY.md section 8)" % k)
        if self.losses_to_use.get("triplet", False) and self.triplet_cfg.get("p", 2) != 2:
            raise L.PcrError("triplet_loss: p = %r; the distance kernels implement p = 2 only" % (self.triplet_cfg.get("p"),))
        if self.sampling == "cartesian" and self._aux_on():
            # (the reference feeds these losses b^2 duplicated rows under cartesian sampling; what they should mean there
            # is undecided)
            raise L.PcrError("sampling='cartesian' trains the match loss only; switch off %s"
                             % ", ".join(k for k in ("cls", "fp", "kl", "triplet") if self.losses_to_use.get(k, False)))

    def _aux_on(self):
        return any(self.losses_to_use.get(k, False) for k in ("cls", "fp", "kl", "triplet"))

    def _object_head(self, name, pooled):
        head = getattr(self, name + "_head")
        if not (isinstance(head, nn.Sequential) and len(head) == 2 and isinstance(head[0], LinearRes)
                and isinstance(head[1], nn.Linear)):
            raise L.PcrError("%s_head must be [LinearRes, Linear] (the reference's configs); got %s"
                             % (name, "None" if head is None else [type(m).__name__ for m in head]
                                if isinstance(head, nn.Sequential) else type(head).__name__))
        if self.training:
            from pcr_amd import train_graph
            return train_graph.rows_head(head, pooled)
        from pcr_amd import rows
        x = pooled.t().contiguous().unsqueeze(0)                 # (1, F, M): channel-major, objects as tokens
        return rows.downsample_points(head, x)[0].t()

    def object_heads(self, h):
        """the per-object heads of cls_forward / fp_forward (reference ReIDNet.py:348-384) on encoded objects h (M, C, N)
        -- siamese_forward's cat(h1, h2), forward_inference's features, the tracker's bank -- -> dict(cls=(M, classes)
        logits or None, fp=(M,) logits or None); a head is evaluated when its loss is switched on.  Pooled once for both
        (get_pooled_feats).  In training mode every launch has a backward (pcr_amd/train_graph.py)."""
        out = dict(cls=None, fp=None)
        want = [k for k in ("cls", "fp") if self.losses_to_use.get(k, False)]
        if not want:
            return out
        L.require_cuda(h)
        if self.training:
            from pcr_amd import train_graph
            pooled = train_graph.pooled_feats(self, h)
        else:
            pooled = self.get_pooled_feats(h)
        for k in want:
            y = self._object_head(k, pooled)
            out[k] = y if k == "cls" else y.reshape(-1)
        return out

    # ------------------------------------------------------------------ mmdet-style entry points
    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)

    def forward_train(self, sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2):
        if self.eval_only:
            exit(0)     # reference behaviour: testing configs stop at the first training iteration (:587-588)
        self._check_losses()
        log_vars, losses = LazyScalars(), {}
        sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2 = self.preprocess_inputs(
            sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2)
        device = sparse_1.device
        xyz1, xyz2, h1, h2 = self.siamese_forward(sparse_1, sparse_2)
        if self.sampling == "cartesian" and self.training:
            # (a training rule: val_step's eval-mode pass and forward_test keep the paired evaluation)
            losses["reid_loss"] = self.match_forward_cartesian(h1, h2, xyz1, xyz2, id_1, id_2, log_vars, device)[1]
            return losses, log_vars
        h1, h2, xyz1, xyz2, match = self.get_match_supervision(h1, h2, xyz1, xyz2, id_1, id_2)
        _, match_loss, o = self.match_forward(h1, h2, xyz1, xyz2, match, log_vars, device)
        loss = match_loss
        if self._aux_on():
            # match + cls + kl + fp + triplet, the reference's order (:632); with the four switches off nothing is launched
            # or added and the match-only step keeps its bits
            from pcr_amd import train_graph
            for extra in train_graph.aux_losses(self, h1, h2, o, torch.cat([label_1, label_2], dim=0),
                                                torch.cat([id_1, id_2], dim=0), match, log_vars):
                if extra is not None:
                    loss = loss + extra
        losses["reid_loss"] = loss
        return losses, log_vars

    def forward_test(self, sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2, size_1, size_2,
                     vis_1, vis_2, *args, **kwargs):
        self._check_losses()
        (sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1, id_2, size_1, size_2, vis_1,
         vis_2) = self.preprocess_inputs_size_vis(sparse_1, sparse_2, dense_1, dense_2, label_1, label_2, id_1,
                                                  id_2, size_1, size_2, vis_1, vis_2)
        device = sparse_1.device
        # (siamese_forward calibrates the split-bf16 guard on the first batch after the weights changed and re-checks it
        # every engine.GUARD_EVERY batches: _guard_tick)
        xyz1, xyz2, h1, h2 = self.siamese_forward(sparse_1, sparse_2)
        h1, h2, xyz1, xyz2, match = self.get_match_supervision(h1, h2, xyz1, xyz2, id_1, id_2)
        match_preds, match_loss, _ = self.match_forward(h1, h2, xyz1, xyz2, match, None, device)
        labels = torch.cat([label_1, label_2], dim=0)
        zero = torch.tensor([0.0])
        # cls, fp and kl as forward_train computes them (no triplet at test time, as in the reference :637-689)
        cls_preds = fp_preds = None
        cls_loss = fp_loss = kl_loss = None
        if self._aux_on():
            import torch.nn.functional as F
            from pcr_amd import train_graph, train_ops
            feats = train_graph._joined(h1, h2)
            preds = self.object_heads(feats)
            cls_preds, fp_preds = preds["cls"], preds["fp"]
            if cls_preds is not None:
                cls_loss = F.cross_entropy(cls_preds, labels.long()) * self.alpha["cls"]
            if fp_preds is not None:
                fp_loss = self.bce(fp_preds, (labels > 9).float()) * self.alpha["fp"]
            if self.losses_to_use.get("kl", False):
                st = train_graph.aux_state(self, feats.device)
                kl_loss = train_ops.KlPairs.apply(feats, match.to(torch.int32), st.info)[0] * self.alpha["kl"]
        results = OrderedDict()
        results["val_dense_loss"] = zero.clone()
        results["val_fp_loss"] = zero.clone() if fp_loss is None else torch.tensor([fp_loss])
        results["val_match_loss"] = torch.tensor([match_loss])
        results["val_shape_loss"] = zero.clone()
        results["val_cls_loss"] = zero.clone() if cls_loss is None else torch.tensor([cls_loss])
        results["val_kl_loss"] = zero.clone() if kl_loss is None else torch.tensor([kl_loss])
        results["val_match_preds"] = match_preds
        results["val_match_gt"] = match
        results["val_cls_preds"] = cls_preds
        results["val_cls_gt"] = labels
        results["val_fp_preds"] = fp_preds
        results["val_fp_gt"] = (labels > 9).float()
        results["match_classes"] = torch.cat([label_1.unsqueeze(1), label_2.unsqueeze(1)], dim=1)
        results["is_fp"] = torch.logical_or(label_1 > 9, label_2 > 9)
        results["num_points"] = torch.cat([size_1.unsqueeze(1), size_2.unsqueeze(1)], dim=1)
        results["val_vis_gt_all"] = torch.cat([vis_1.unsqueeze(1), vis_2.unsqueeze(1)], dim=1)
        return [results]

    def validate_step(self, batch, book, count=None):
        """forward_test's scoring half for a device-side book (pcr_amd.matchbook.MatchBook): the same inputs, the same
        encode + match launches and so the same logits, but the batch's pairs go into the book's table by one launch
        (`book.add`; the per-object heads, when their losses are on, by `book.add_objects`) instead of coming back as
        tensors.  No host tensor is built and nothing is returned that forces a read, so a step can be captured in a HIP
        graph and replayed (the split-bf16 guard measures nothing inside a capture: calibrate before, as for every
        captured entry point).  count: a (1,) int32 device tensor -- only the first count pairs of a padded batch are
        scored.  The validation losses stay with forward_test."""
        self._check_losses()
        if not self.losses_to_use["match"]:
            raise L.PcrError("validate_step scores the match logits; losses_to_use['match'] is off")
        keys = ("sparse_1", "sparse_2", "dense_1", "dense_2", "label_1", "label_2", "id_1", "id_2", "size_1", "size_2",
                "vis_1", "vis_2")
        (sparse_1, sparse_2, _, _, label_1, label_2, id_1, id_2, size_1, size_2, vis_1,
         vis_2) = self.preprocess_inputs_size_vis(*(batch[k] for k in keys))
        xyz1, xyz2, h1, h2 = self.siamese_forward(sparse_1, sparse_2)
        h1, h2, xyz1, xyz2, match = self.get_match_supervision(h1, h2, xyz1, xyz2, id_1, id_2)
        with self._at_level(self.precision_level()):
            match_preds, _ = self._match_logits(h1, h2, xyz1, xyz2)
        if self._aux_on():
            from pcr_amd import train_graph
            preds = self.object_heads(train_graph._joined(h1, h2))
            labels = torch.cat([label_1, label_2], dim=0)
            if preds["cls"] is not None or preds["fp"] is not None:
                book.add_objects(cls_logits=preds["cls"], cls_gt=None if preds["cls"] is None else labels,
                                 fp_logits=preds["fp"], fp_gt=None if preds["fp"] is None else (labels > 9).float(),
                                 count=count, period=h1.shape[0])
        book.add(logit=match_preds, gt=match, cls=torch.stack([label_1, label_2], dim=1),
                 num_points=torch.stack([size_1, size_2], dim=1), vis=torch.stack([vis_1, vis_2], dim=1), count=count)

    @staticmethod
    def _parse_losses(losses):
        """mmdet BaseDetector._parse_losses: mean every entry, sum those whose key contains 'loss',
        all-reduce the logged scalars across ranks when torch.distributed is initialised."""
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError("%s is not a tensor or list of tensors" % name)
        loss = sum(v for k, v in log_vars.items() if "loss" in k)
        log_vars["loss"] = loss
        # mmdet reduces and reads every entry on its own (one all-reduce + one .item() each); here the entries travel as
        # ONE stacked tensor: one all-reduce, one asynchronous copy, read on first access (pcr_amd/lazylog.py)
        import torch.distributed as dist
        from pcr_amd import lazylog
        names = list(log_vars.keys())
        stacked = torch.stack([log_vars[k].detach().reshape(()).float() for k in names])
        log_vars = LazyScalars()
        if dist.is_available() and dist.is_initialized():
            if lazylog.DEFER_REDUCE:
                # under pcr_amd.train.Trainer: averaged in the tail of the gradient bucket -- no collective inside the
                # (capturable) forward + backward, one all-reduce per iteration in total
                log_vars.add_device(names, stacked, reduce=True)
                return loss, log_vars
            stacked = stacked.clone()
            dist.all_reduce(stacked.div_(dist.get_world_size()))
        log_vars.add_device(names, stacked)
        return loss, log_vars

    def train_step(self, data, optimizer):
        losses, log_vars_train = self(**data)
        loss, log_vars = self._parse_losses(losses)
        log_vars.update(log_vars_train)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data["sparse_1"]))

    def val_step(self, data, optimizer=None):
        losses, _ = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data["sparse_1"]))

    def extract_feat(self, *args, **kwargs):
        raise NotImplementedError

    def show_result(self):
        raise NotImplementedError

    def aug_test(self, *args, **kwargs):
        raise NotImplementedError

    def simple_test(self, *args, **kwargs):
        raise NotImplementedError

    def init_weights(self):
        pass
