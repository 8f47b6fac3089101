"""Set-abstraction and feature-propagation layers of the reference's "Point-Transformer"
backbone (STNet-style PointNet++ with linear attention), re-implemented as thin parameter
holders over the fused gfx950 kernels.

Reference: mmdet3d/models/pointnet2_utils.py -- Self_Attention :55-114, sample_and_group_edge
:242-288, PointNetSetAbstractionEdgeSA :309-360, FP_SA :362-437, PointNetFeaturePropagationSA
:439-473.  Parameter names/shapes are identical so reference checkpoints load unchanged
(SURVEY.md Appendix A), including the FP layers' never-used mlp_convs / mlp_bns.

Forward = three launches per SA layer (pcr_knn_prefix_f32, pcr_sa_mlp_f32, pcr_attn_kv/apply)
and two per FP layer; the unfused chain of the reference (distance matrix, argsort, gathers,
cat, conv/bn/relu, max, einsum attention) never materialises.
"""
import torch
import torch.nn as nn

from pcr_amd import engine
from pcr_amd import _lib as L


# ---- the model path's function-level samplers / groupers (reference pointnet2_utils.py:116-240), on the HIP ops ----
def random_point_sample(xyz, npoint):
    """prefix sampling: indices 0..npoint-1 of every cloud (:139-149) -> (B,npoint) int64"""
    return torch.arange(npoint, dtype=torch.long, device=xyz.device).repeat(xyz.size(0), 1)


def farthest_point_sample(xyz, npoint, start=None):
    """(:116-137) FPS with a RANDOM first pick (torch.randint, as in the reference; pass `start` (B,) to fix it),
    ties to the lowest index -> (B,npoint) int64"""
    L.require_cuda(xyz)
    L.require_f32(xyz)
    xyz = xyz.contiguous()
    B, N, _ = xyz.shape
    if start is None:
        start = torch.randint(0, N, (B,), dtype=torch.long).to(xyz.device)
    if not start.is_cuda and start.numel() and (int(start.min()) < 0 or int(start.max()) >= N):
        raise L.PcrError("farthest_point_sample: start index outside [0, %d)" % N)
    # (a start tensor already on the device is not read back: the kernel clamps an out-of-range entry to point 0)
    start = start.to(device=xyz.device, dtype=torch.int32).contiguous()
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
    L.run.pcr_fps_py_f32(xyz, temp, start, idx, B, N, npoint, L.stream_ptr())
    return idx.long()


def query_ball_point(radius, nsample, xyz, new_xyz):
    """(:218-240) first `nsample` points with d <= radius^2 (expanded-form distance) in index order, padded with the
    first -> (B,S,nsample) int64"""
    L.require_cuda(xyz, new_xyz)
    L.require_f32(xyz, new_xyz)
    xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    idx = torch.empty((B, S, nsample), dtype=torch.int32, device=xyz.device)
    L.run.pcr_query_ball_point_f32(new_xyz, xyz, idx, B, N, S, radius, nsample, L.stream_ptr())
    return idx.long()


def knn_point(nsample, xyz, new_xyz):
    """(:205-216) the nsample nearest points of every centre -> (B,S,nsample) int64 (ascending distance; the reference
    leaves the order inside a K-set to an unstable argsort, its consumer is a max over K)"""
    from mmdet3d.ops.point_ops import knn
    return knn(nsample, xyz.contiguous(), new_xyz.contiguous(), False).transpose(1, 2).contiguous().long()


def index_points(points, idx):
    """(:151-167) points (B,N,C), idx (B,S) or (B,S,K) -> (B,S[,K],C), through the HIP gather ops"""
    from mmdet3d.ops.point_ops import gather_points, grouping_operation
    feats = points.transpose(1, 2).contiguous()
    i32 = idx.to(torch.int32).contiguous()
    if idx.dim() == 2:
        return gather_points(feats, i32).transpose(1, 2).contiguous()
    return grouping_operation(feats, i32).permute(0, 2, 3, 1).contiguous()


class _Planned(nn.Module):
    """caches the packed weight image of a module; rebuilt when a parameter changes or moves"""

    def _plan(self, device, build):
        if self.training:
            raise L.PcrError(
                "%s: the fused HIP path implements eval-mode inference (BatchNorm folded from running "
                "statistics); call .eval() -- training kernels are listed as next work in DESIGN.md"
                % type(self).__name__)
        key = (str(device), engine.param_version(self))
        if getattr(self, "_plan_key", None) != key:
            object.__setattr__(self, "_plan_obj", build(device))
            object.__setattr__(self, "_plan_key", key)
        return self._plan_obj


def _attn_holder(m, pos_name, d_model, c_q, c_k, c_pos_out, c_ff_in, out_dim):
    setattr(m, pos_name, nn.Sequential(nn.Linear(3, d_model), nn.ReLU(), nn.Linear(d_model, c_pos_out)))
    m.q_proj = nn.Linear(c_q, d_model, bias=False)
    m.k_proj = nn.Linear(c_k, d_model, bias=False)
    m.v_proj = nn.Linear(c_k, d_model, bias=False)
    m.merge = nn.Linear(d_model, d_model, bias=False)
    m.mlp = nn.Sequential(nn.Linear(c_ff_in, d_model * 2, bias=False), nn.ReLU(True),
                          nn.Linear(d_model * 2, out_dim, bias=False))
    m.norm1 = nn.LayerNorm(d_model)
    m.norm2 = nn.LayerNorm(out_dim)


class Self_Attention(_Planned):
    """feat (B,C,N), xyz (B,N,3) -> (B,C,N): linear self-attention with xyz position encoding on
    q, k and v, LayerNorm, feed-forward on [feat, msg], LayerNorm, residual."""

    def __init__(self, d_model, nhead, attention="linear"):
        super().__init__()
        self.dim = d_model // nhead
        self.nhead = nhead
        _attn_holder(self, "pos_mlp", d_model, d_model, d_model, d_model, d_model * 2, d_model)

    def forward(self, feat, xyz, mask=None):
        assert mask is None, "masks are never passed by the ReID model path"
        plan = self._plan(feat.device, lambda dev: engine.AttnPlan(self, "pos_mlp", dev, self.nhead,
                                                                   q_pos=True, k_pos=True, residual=True))
        feat = feat.contiguous()
        xyz = xyz.contiguous()
        return plan.run(feat, xyz, feat, xyz)


class PointNetSetAbstractionEdgeSA(_Planned):
    def __init__(self, npoint, radius, nsample, mlp, sampling, use_xyz=True, group_all=False, use_knn=False):
        super().__init__()
        if group_all:
            raise NotImplementedError("group_all SA layers are never built by the ReID backbone (backbone_net.py:50-81)")
        if sampling not in ("RANDOM", "FPS"):
            raise ValueError("sampling must be 'RANDOM' or 'FPS'")
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.use_xyz, self.sampling, self.use_knn, self.group_all = use_xyz, sampling, use_knn, group_all
        mlp = list(mlp)
        if use_xyz:
            mlp[0] += 3
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = mlp[0]
        for out_channel in mlp[1:]:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel
        self.self_attention = Self_Attention(last, 2, "linear")

    def shares_knn_with(self, nxt, n, numpoints, numpoints_next):
        """may this level and the next one take their neighbours from ONE search (engine.knn_prefix2)?  This level keeps
        all n points (so the next level queries the same cloud), both sample a prefix and search by kNN, and the next
        level asks for at least as many neighbours of at most as many centres."""
        return (isinstance(nxt, PointNetSetAbstractionEdgeSA) and self.sampling == "RANDOM" and self.use_knn and
                nxt.sampling == "RANDOM" and nxt.use_knn and numpoints == n and numpoints_next <= numpoints and
                self.nsample <= nxt.nsample <= min(64, n))

    def forward(self, xyz, points, numpoints, knn_idx=None):
        """xyz (B,N,3); points (B,D,N) or None -> (new_xyz (B,S,3), (B,D',S)); S = numpoints
        knn_idx: this level's (B,S,K) neighbour indices when the caller has already searched (engine.knn_prefix2)"""
        plan = self._plan(xyz.device, lambda dev: engine.SaPlan(list(self.mlp_convs), list(self.mlp_bns), dev, mode=0))
        xyz = xyz.contiguous()
        points = None if points is None else points.contiguous()
        if self.sampling == "RANDOM" and self.use_knn:      # the configuration every ReID config builds
            idx = knn_idx if knn_idx is not None else engine.knn_prefix(xyz, numpoints, self.nsample)
            assert idx.shape == (xyz.shape[0], numpoints, self.nsample)
            pooled = engine.guarded(lambda: plan.run(xyz, points, idx))   # folded BatchNorm: f32 from guard level 1
            new_xyz = xyz[:, :numpoints].contiguous()
            return new_xyz, self.self_attention(pooled, new_xyz)
        # the dormant branches of sample_and_group_edge (:262-272): FPS centres and / or ball-query groups
        centre = (farthest_point_sample(xyz, numpoints) if self.sampling == "FPS"
                  else random_point_sample(xyz, numpoints)).to(torch.int32).contiguous()
        new_xyz = index_points(xyz, centre)
        idx = (knn_point(self.nsample, xyz, new_xyz) if self.use_knn
               else query_ball_point(self.radius, self.nsample, xyz, new_xyz)).to(torch.int32).contiguous()
        pooled = engine.guarded(lambda: plan.run(xyz, points, idx, centre_idx=centre))
        return new_xyz, self.self_attention(pooled, new_xyz)


class FP_SA(_Planned):
    """fine <- coarse linear cross-attention (keys without, values with position encoding), no residual"""

    def __init__(self, last_channel, feat1_dim, feat2_dim, d_model, out_dim, nhead, attention="linear"):
        super().__init__()
        self.dim = d_model // nhead
        self.nhead = nhead
        _attn_holder(self, "pos_mlp2", d_model, feat1_dim, feat2_dim, feat2_dim, feat1_dim + d_model, out_dim)
        self._final = None

    def fuse_final_conv(self, conv):
        """let the trailing 1x1 Conv1d (Pointnet_Backbone.cov_final) run inside the same launch"""
        object.__setattr__(self, "_final", conv)
        object.__setattr__(self, "_plan_key", None)

    def forward(self, feat1, xyz1, feat2, xyz2, mask=None):
        assert mask is None
        plan = self._plan(feat1.device, lambda dev: engine.AttnPlan(self, "pos_mlp2", dev, self.nhead, q_pos=False,
                                                                    k_pos=False, residual=False, final=self._final))
        return plan.run(feat1.contiguous(), xyz1.contiguous(), feat2.contiguous(), xyz2.contiguous())

    def _plan(self, device, build):
        key = (str(device), engine.param_version(self),
               None if self._final is None else engine.param_version(self._final))
        if self.training:
            raise L.PcrError("FP_SA: the fused HIP path implements eval-mode inference; call .eval()")
        if getattr(self, "_plan_key", None) != key:
            object.__setattr__(self, "_plan_obj", build(device))
            object.__setattr__(self, "_plan_key", key)
        return self._plan_obj


class PointNetFeaturePropagationSA(nn.Module):
    def __init__(self, mlp, mlp_inte):
        super().__init__()
        # constructed but never used by forward, exactly as in the reference (:442-449): they exist
        # only so that checkpoints (and DDP's unused-parameter handling) see the same tensors
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = mlp[0]
        for out_channel in mlp[1:]:
            self.mlp_convs.append(nn.Conv1d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last = out_channel
        self.interpolation = FP_SA(last_channel=mlp_inte[0], feat1_dim=mlp_inte[1], feat2_dim=mlp_inte[2],
                                   d_model=mlp_inte[3], out_dim=mlp_inte[4], nhead=2, attention="linear")

    def forward(self, xyz1, xyz2, points1, points2):
        return self.interpolation(points1, xyz1, points2, xyz2)
