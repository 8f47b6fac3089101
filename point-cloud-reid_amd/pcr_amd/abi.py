"""The C ABI of libpcr_hip.so (include/pcr.h) as Python sees it, in ONE place: the parameter blocks, the two device-table
record layouts, and the signature of every entry point.  `_lib.load()` applies SIGNATURES to the loaded library;
tests/test_abi.py holds every line of this file against the header (prototypes by a parse, layouts by a compiled
sizeof / offsetof probe)."""
import ctypes

import numpy as np
import torch

_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long": ctypes.c_long}
_POINTERS = {"iptr": torch.int32, "fptr": torch.float32, "dptr": torch.float64, "lptr": torch.int64, "ptr": None}


def _block(name, decl):
    """ctypes mirror of a pcr.h parameter block.  `decl` follows the header's struct body, one `type field field ...`
    group per `;`.  A data pointer is named by what it points at: iptr = int *, fptr = float *, dptr = double *, lptr =
    long long *, ptr = void *; kind[n] = an array of n.  Every pointer is a c_void_p in the layout (the launches fill them
    with addresses: `fill`, `_lib._p`); the class keeps the element types as ELEM = {pointer field: torch dtype or None}."""
    fields, elem = [], {}
    for group in decl.split(";"):
        ty, *names = group.split()
        base, _, n = ty.partition("[")
        if base in _POINTERS:
            elem.update(dict.fromkeys(names, _POINTERS[base]))
        ct = ctypes.c_void_p if base in _POINTERS else _CTYPES[base]
        fields += [(f, ct * int(n[:-1]) if n else ct) for f in names]
    return type(name, (ctypes.Structure,), {"_fields_": fields, "ELEM": elem})


def fill(p, tensors, sizes, required=(), who="pcr_amd"):
    """Checks the dict `tensors` over the pointer fields of the block `p` against the block's element types and the element
    counts `sizes`, writes the addresses into `p` (None and an empty tensor: NULL) and returns it.  What is wrong with the
    call itself comes before where a tensor lives, so every refusal but the last can be met without a device; a field not
    named in `required` may be None (the library's own NULL checks stay the authority).  Nothing here reads the device,
    allocates or converts: it is legal inside a graph capture."""
    from . import _lib as L
    elem = type(p).ELEM
    for k in tensors:
        if k not in elem:
            L.refuse(who, "unknown tensor %r" % (k,))
    for k, x in tensors.items():
        if x is not None and not isinstance(x, torch.Tensor):
            L.refuse(who, "%s must be a tensor" % k)
    for k in required:
        if tensors.get(k) is None and sizes[k] != 0:
            L.refuse(who, "%s is missing" % k)
    for k, x in tensors.items():
        if x is not None and elem[k] is not None and x.dtype != elem[k]:
            L.refuse(who, "%s must be a %s tensor, got %s" % (k, elem[k], x.dtype))
    for k, x in tensors.items():
        if x is not None and (x.numel() != sizes[k] or not x.is_contiguous()):
            L.refuse(who, "%s must be contiguous and hold %d elements, got %s" % (k, sizes[k], tuple(x.shape)))
    L.require_cuda(*tensors.values())
    for k, x in tensors.items():
        setattr(p, k, x.data_ptr() if x is not None and x.numel() else None)
    return p


# ---- section A5 (pcr_bank) ----
BankParams = _block("BankParams", """
    int C D W frame_limit replace_all reset_on_match propagate;
    iptr lengths; fptr boxes scores; iptr labels ids steps misses next_id info;
    iptr track_to_det det_to_track det_labels det_lengths; fptr det_boxes det_scores; iptr born kill; fptr carry;
    iptr src det_slot det_id""")

# ---- section A3 (pcr_assoc_multi, pcr_assoc_decode) ----
AssocMultiParams = _block("AssocMultiParams", """
    int T D dd td cap kind reduce; float dist_max dist_penalty fill; fptr logits; iptr pairs count;
    fptr det_dec trk_dec dist; ptr ws; fptr cost; iptr det_choice trk_choice""")
AssocDecodeParams = _block("AssocDecodeParams", """
    int T D dd td reduce born_dec kill_dec; float fill; fptr cost; iptr col4row row4col solver_info det_choice trk_choice;
    iptr track_to_det det_to_track det_decision track_decision born kill info""")

# ---- section A7 (pcr_truth) ----
TruthParams = _block("TruthParams", """
    int C D G gt_cap skip_empty forced; iptr ids slot_gt slot_tte gt_last stats col4row row4col info; fptr cost thresh;
    iptr gt_labels gt_ids gt_tte det_labels track_to_det det_to_track born kill;
    iptr det_gt true_t2d true_d2t det_truth track_truth det_slot det_id""")

# ---- section A8 (pcr_rank, pcr_rank_acc) ----
RankParams = _block("RankParams", """
    int Q G K; fptr scores; iptr query_ids gallery_ids exclude topk_idx; fptr topk_score; iptr n_cand n_true first_hit;
    fptr ap; iptr info""")
RankAccParams = _block("RankAccParams", """
    int Q G nranks; int[8] ranks; iptr n_true first_hit info; fptr ap; iptr valid counts; dptr sums""")

# ---- section A9 (pcr_ident, pcr_ident_close) ----
IdentParams = _block("IdentParams", """
    int D G gt_cap gt_rows id_cap; iptr det_labels det_gt det_id gt_labels gt_ids; fptr cost; iptr cooc gt_track totals;
    dptr dist_sum""")
IdentCloseParams = _block("IdentCloseParams", """
    int gt_rows id_cap max_rows max_cols; iptr cooc gt_track totals; dptr dist_sum; iptr flags counts row_list col_list;
    fptr cost; iptr col4row info id_map; lptr table; dptr dist_total""")

# ---- section A10 (pcr_pair_head_params) ----
PairHeadParams = _block("PairHeadParams", """
    int M F n groups; long P; fptr emb u v; iptr pairs; fptr w2p gn1_g gn1_b gn2_g gn2_b w_out b_out logits""")

# ---- section A11 (pcr_bank_rules, pcr_scene_log) ----
BankRulesParams = _block("BankRulesParams", """
    int C D W frame_limit replace_all reset_on_match dd td match_rule; int[4] det_rule trk_rule trk_kind;
    iptr lengths; fptr boxes scores; iptr labels ids steps misses next_id;
    iptr track_to_det det_to_track det_labels det_lengths; fptr det_boxes det_scores; iptr det_decision track_decision;
    fptr carry; iptr src det_slot det_id info; iptr out_valid out_ids out_labels; fptr out_scores out_boxes; iptr out_flags""")
SceneLogParams = _block("SceneLogParams", """
    int rows_max R W; iptr in_valid in_ids in_labels; fptr in_scores in_boxes; iptr in_flags;
    iptr frame id label flags; fptr score box; iptr cursor dropped frame_no""")

# ---- section A13 (pcr_match) ----
MatchParams = _block("MatchParams", """
    int P; fptr logit gt; iptr cls num_points vis count; lptr table; iptr info""")

# ---- section A6 (pcr_store_tables) ----
StoreTables = _block("StoreTables", """
    int num_objects num_classes;
    iptr obj_cls obj_fp obj_id nums_off nums_rows bucket_off bucket_rows pool_off pool_objs""")

# ---- section B (pcr_sa_params, pcr_attn_params, pcr_head_params) ----
SaParams = _block("SaParams", """
    int mode B N S K D c1 c2 c3; fptr xyz feat; iptr idx centre_idx; fptr[3] wp scale shift; fptr wa wpq;
    fptr[2] wps shift_pad; iptr cnt tile_ws; fptr pq_ws; int pq_ready feat_point_major out_point_major; fptr out wa_packed;
    int precision; fptr[2] wps_bf; fptr wa_shift_packed row_tab; iptr claim_ws; int pq_has_xyz""")
AttnParams = _block("AttnParams", """
    int B Lq Sk c1 c2 d cout nhead q_pos residual; fptr feat_q xyz_q feat_k xyz_k; iptr kv_index q_index; fptr pos0_w pos0_b;
    fptr wq bq wkv bkv wmerge wmlp0 wmlp2 ln1_g ln1_b ln2_g ln2_b wfinal bfinal; int cfinal;
    fptr wkv_wide bkv_wide wmerge_packed kv out; int precision; fptr wq_bf wmlp0_bf wmlp2_bf wfinal_bf; int kv_splits;
    fptr kv_part wkv_bf wmlp0_bf_xpad pool_out""")
HeadParams = _block("HeadParams", """
    int P C L groups; fptr o w1 w2 gn1_g gn1_b gn2_g gn2_b w_out b_out pooled logits w1t w2t""")
LiveParams = _block("LiveParams", "iptr count; int period offset")     # pcr_live: the gate of the _live launches

# ---- section C (pcr_tdense_fwd / _bwd, pcr_bn_fwd_fin / _bwd_fin, pcr_reduce_job, pcr_linattn, pcr_attn_tail / _head) ----
_TFwd = _block("_TFwd", """
    int B cin1 cin2 cout L; fptr x x2 isc ish; int in_relu; fptr wp bias res; int out_relu; fptr y stats; int pool_K;
    fptr pool_gamma pool_ymax; iptr pool_arg""")
_TBwd = _block("_TBwd", """
    int B cin1 cin2 cout L; fptr g y; int dy_mode; fptr ka kb kc; iptr argmax; fptr pooled; int K S;
    fptr x x2 isc ish iinv; int in_relu; fptr wpT dx dx2 dstats dwp dbp; long part_stride; int precision; fptr wpT_bf""")
_BnFwd = _block("_BnFwd", """
    fptr part; int nparts C; double R; fptr gamma beta; float eps momentum;
    fptr running_mean running_var scale shift inv_scale mean invstd shift0; int shift0_stride""")
_BnBwd = _block("_BnBwd", """
    fptr part; int nparts C; double R; fptr gamma mean invstd ka kb kc dgamma dbeta centre""")
_ReduceJob = _block("_ReduceJob", "fptr part out; long stride; int nparts rows cols ld")
_LinAttnP = _block("_LinAttnP", """
    int B Lq Sk d H; float eps; fptr q k v; long q_bs k_bs v_bs; fptr out A ks dout dq dk dv; long dq_bs dk_bs dv_bs;
    int kv_roll""")
_AttnTailP = _block("_AttnTailP", """
    int B L d c1 hid out residual; float eps; fptr msg res wm w0 w2 wmT w0T w2T g1 b1 g2 b2 outp dout dmsg dres parts;
    long part_stride; int precision fwd_precision""")
_AttnHeadP = _block("_AttnHeadP", """
    int B L c hd d np src; fptr x xyz p1 p2 c1 c2 p2T; fptr[3] w wT; fptr outp dout dx parts; long part_stride;
    int precision fwd_precision""")

# the header's name of every block (what the layout test compiles against)
BLOCKS = {"pcr_assoc_multi": AssocMultiParams, "pcr_assoc_decode": AssocDecodeParams, "pcr_bank": BankParams,"pcr_truth": TruthParams, "pcr_store_tables": StoreTables, "pcr_sa_params": SaParams, "pcr_attn_params": AttnParams, "pcr_head_params": HeadParams,
          "pcr_live": LiveParams, "pcr_rank": RankParams, "pcr_rank_acc": RankAccParams,
          "pcr_ident": IdentParams, "pcr_ident_close": IdentCloseParams,
          "pcr_tdense_fwd": _TFwd, "pcr_tdense_bwd": _TBwd, "pcr_bn_fwd_fin": _BnFwd, "pcr_bn_bwd_fin": _BnBwd,
          "pcr_reduce_job": _ReduceJob, "pcr_linattn": _LinAttnP, "pcr_attn_tail": _AttnTailP,
          "pcr_attn_head": _AttnHeadP}

# ---- records of the DEVICE tables (built with numpy on the host, uploaded as bytes) ----
pcr_pack_desc = np.dtype([("w", "<u8"), ("out", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("kind", "<i4"),
                          ("reserved", "<i4")])
pcr_opt_tensor = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"),
                           ("bc2_sqrt", "<f4"), ("decay", "<f4"), ("one_m_beta1", "<f4"), ("beta2", "<f4"),
                           ("one_m_beta2", "<f4"), ("eps", "<f4"), ("pad_", "<f4")])
TABLES = {"pcr_pack_desc": pcr_pack_desc, "pcr_opt_tensor": pcr_opt_tensor}


# ---- pointer parameters that take a tensor ----
class _TensorPtr:
    """argtype of a `float *` / `int *` parameter.  Accepts None (NULL), a device tensor of `dtype` on the current device
    (strided views included: the callers pass an explicit ld), a Python int address (`data_ptr() + 4 * off`), and
    anything ctypes itself takes for a void pointer (c_void_p, byref, arrays: host images).  Any other tensor raises,
    which ctypes reports as ArgumentError with the argument's index before the call is made.  A tensor of another dtype
    that is meant to go in (index bits in a float table) takes the explicit unchecked route, `_lib.ptr(t)`."""
    dtype = None

    @classmethod
    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            if v.dtype is not cls.dtype:
                raise TypeError("expected a %s tensor, got %s" % (cls.dtype, v.dtype))
            if not v.is_cuda or v.device.index != torch.cuda.current_device():
                raise TypeError("expected a tensor on the current GPU, got one on %s" % v.device)
            return ctypes.c_void_p(v.data_ptr())
        if v is None:
            return None
        if isinstance(v, int):
            return ctypes.c_void_p(v)
        return ctypes.c_void_p.from_param(v)


class FloatPtr(_TensorPtr):
    dtype = torch.float32


class IntPtr(_TensorPtr):
    dtype = torch.int32


# ---- every prototype of pcr.h: "<return> <one letter per parameter>" ----
#   return     s status int (0 = ok; `_lib.run.<name>` raises on anything else)   i int   l long   c char *
#   parameter  i int   f float   l long   S stream   F float *   I int *   P any other pointer (double *, long long *,
#              a device table)   <Block> pointer to that parameter block
SIGNATURES = {
    "pcr_abi_version": "i ",
    "pcr_status_string": "c i",
    # A. point ops
    "pcr_fps_f32": "s FFIiiiS",
    "pcr_fps_dist_f32": "s FFIiiiS",
    "pcr_pairwise_sqdist_f32": "s FFFiiiiiS",
    "pcr_ball_query_f32": "s FFIiiiffiS",
    "pcr_ball_query_cnt_f32": "s FFIIiiiffiS",
    "pcr_ball_query_rows_floats": "l iii",
    "pcr_ball_query_rows_ok": "i iif",
    "pcr_ball_query_rows_f32": "s FFIIFiiiffiS",
    "pcr_fps_ball_query_rows_ok": "i iii",
    "pcr_fps_ball_query_rows_f32": "s FFIFIFiiifiS",
    "pcr_fps_py_f32": "s FFIIiiiS",
    "pcr_query_ball_point_f32": "s FFIiiifiS",
    "pcr_knn_f32": "s FFIFiiiiS",
    "pcr_gather_fwd_f32": "s FIFiiiiS",
    "pcr_gather_bwd_f32": "s FIFiiiiS",
    "pcr_group_fwd_f32": "s FIFiiiiiS",
    "pcr_group_bwd_f32": "s FIFiiiiiS",
    "pcr_three_nn_f32": "s FFFIiiiS",
    "pcr_three_interp_fwd_f32": "s FIFFiiiiS",
    "pcr_three_interp_bwd_f32": "s FIFFiiiiS",
    # A2. points in boxes, crops
    "pcr_box_frames_f32": "s FFiS",
    "pcr_points_in_boxes_batch_f32": "s FFIiiiS",
    "pcr_points_in_boxes_f32": "s FFIiiiS",
    "pcr_crop_boxes_ok": "i iiii",
    "pcr_crop_boxes_f32": "s FiFIPFIiiiiiiS",
    # A3. association
    "pcr_assoc_pairs_ok": "i iiii",
    "pcr_assoc_pairs_i32": "s IIIIIIiiiiiS",
    "pcr_assoc_cost_f32": "s FIIFFFfffFiiiS",
    "pcr_lsa_ok": "i iii",
    "pcr_lsa_f32": "s FIIFFIiiiS",
    "pcr_lsa_blocks_ok": "i iii",
    "pcr_lsa_blocks_f32": "s FIIIIFFIiiiS",
    "pcr_assoc_blocks_i32": "s IIIIiiiiiS",
    "pcr_assoc_multi_ok": "i iiiii",
    "pcr_assoc_multi_ws_bytes": "i iiii",
    "pcr_assoc_cost_multi_f32": "s <AssocMultiParams>S",
    "pcr_assoc_decode_i32": "s <AssocDecodeParams>S",
    # A4. box overlap and suppression
    "pcr_nearest_bev_f32": "s FFiS",
    "pcr_bev_frames_f32": "s FFiS",
    "pcr_iou_bev_f32": "s FFFiiiS",
    "pcr_nms_ok": "i i",
    "pcr_nms_ws_bytes": "i i",
    "pcr_nms_f32": "s FFFIIIIPiiiS",
    "pcr_track_nms_f32": "s FIFFIiS",
    # A5. track state
    "pcr_bank_ok": "i iiiii",
    "pcr_bank_plan_i32": "s <BankParams>S",
    "pcr_bank_move_f32": "s IFFFFiiiiS",
    "pcr_bank_dist_f32": "s FIFFFiiiS",
    "pcr_bank_retire_i32": "s IIIIiS",
    # A6. crop store
    "pcr_store_gather_f32": "s FPiIIIPFIIiiS",
    "pcr_store_train_pairs_i32": "s <StoreTables>IIIPIIIIiS",
    # A7. ground truth
    "pcr_truth_ok": "i iiiii",
    "pcr_truth_cost_f32": "s FIFIIFFiiiiS",
    "pcr_truth_decide_i32": "s <TruthParams>S",
    "pcr_truth_record_i32": "s <TruthParams>S",
    # A8. ranking a gallery
    "pcr_rank_ok": "i iiii",
    "pcr_rank_scores_f32": "s FIIFiiiS",
    "pcr_rank_gallery_f32": "s <RankParams>S",
    "pcr_rank_accumulate": "s <RankAccParams>S",
    # A9. identity preservation
    "pcr_ident_ok": "i iiiiiii",
    "pcr_ident_record_i32": "s <IdentParams>S",
    "pcr_ident_compact_f32": "s <IdentCloseParams>S",
    "pcr_ident_score_i32": "s <IdentCloseParams>S",
    # A10. pair head over embeddings (the block is passed as a plain pointer: byref(PairHeadParams))
    "pcr_pair_head_ok": "i ii",
    "pcr_pair_head_f32": "s P<LiveParams>FS",
    # A11. the updater as configured, the scene log (plain pointers as A10: byref(BankRulesParams / SceneLogParams))
    "pcr_bank_rules_ok": "i iiiii",
    "pcr_bank_plan_rules_i32": "s PS",
    "pcr_scene_log_ok": "i iii",
    "pcr_scene_log_append_i32": "s PS",
    # A12. ranking a wide gallery
    "pcr_rank_wide_ok": "i iii",
    "pcr_rank_fill_f32": "s FiiS",
    "pcr_rank_scatter_f32": "s FIIFiiiiiS",
    "pcr_rank_wide_f32": "s <RankParams>S",
    # A13. scoring a validation split (the block is passed as a plain pointer, as A10: byref(MatchParams))
    "pcr_match_ok": "i iii",
    "pcr_match_record_i64": "s PS",
    "pcr_match_record_objects_i64": "s FIFFIPIiiiS",
    # B. fused model kernels
    "pcr_knn_prefix_f32": "s FIiiiiS",
    "pcr_knn_prefix2_f32": "s FIIiiiiiiS",
    "pcr_packed_weight_floats": "l ii",
    "pcr_pack_weight_f32": "s FiiF",
    "pcr_packed_weight_bf16_floats": "l ii",
    "pcr_pack_weight_bf16x2_f32": "s FiiF",
    "pcr_sa_mlp_f32": "s <SaParams>S",
    "pcr_sa_claim_ws_ints": "l iiiiii",
    "pcr_sa_tile_ws_ints": "l iiiii",
    "pcr_sa_krow_uses_tiles": "i iiiii",
    "pcr_sa_uses_row_table": "i iiiii",
    "pcr_sa_launch_form": "i <SaParams>I",
    "pcr_dense_pm_f32": "s FFFiiiiiS",
    "pcr_dense_pm_prec_f32": "s FFFiiiiiiS",
    "pcr_dense_pm_xyz_f32": "s FFFFFiiiiiiiiS",
    "pcr_sa_tables_take_xyz": "i iiiiiii",
    "pcr_attn_kv_floats": "l i",
    "pcr_attn_kv_splits": "i iii",
    "pcr_attn_kv_f32": "s <AttnParams>S",
    "pcr_attn_apply_f32": "s <AttnParams>S",
    "pcr_attn_apply_pool_ok": "i <AttnParams>",
    "pcr_attn_live_ok": "i <AttnParams>",
    "pcr_attn_kv_live_f32": "s <AttnParams><LiveParams>S",
    "pcr_attn_apply_live_f32": "s <AttnParams><LiveParams>S",
    "pcr_attn_launch_form": "i <AttnParams><LiveParams>iI",
    "pcr_pool_head_f32": "s <HeadParams>S",
    "pcr_pool_head_live_f32": "s <HeadParams><LiveParams>FS",
    "pcr_pool_both_f32": "s FFiiiS",
    "pcr_channel_max_f32": "s FFiiiiS",
    "pcr_dense_f32": "s FFFFFiiiiiS",
    "pcr_dense_xpm_f32": "s FFFFFiiiiiS",
    "pcr_dense_gn_f32": "s FFFFFFiiiiiiS",
    "pcr_dense_prec_ok": "i iii",
    "pcr_dense_prec_f32": "s FFFFFiiiiiiS",
    "pcr_dense_gn_prec_f32": "s FFFFFFiiiiiiiS",
    "pcr_dense_xpm_prec_ok": "i iii",
    "pcr_dense_xpm_prec_f32": "s FFFFFiiiiiiS",
    "pcr_max_over_l_f32": "s FFiiiS",
    "pcr_dense_max_ok": "i iii",
    "pcr_dense_max_f32": "s FFFFFiiiiiS",
    "pcr_pack_bmm_f32": "s FFiiS",
    "pcr_dense_bmm_f32": "s FFFiiiiS",
    "pcr_groupnorm_f32": "s FFFFFiiiiiS",
    "pcr_knn_feat_f32": "s FFIiiiilS",
    "pcr_edge_max_f32": "s FFIFfFlFliiiiS",
    "pcr_local_attn_f32": "s FIFiiiiifS",
    # C. training-mode kernels
    "pcr_pack_weight_dev_f32": "s FiiiiFS",
    "pcr_train_groups": "i ii",
    "pcr_train_groups_bwd": "i iiii",
    "pcr_tdense_fwd_groups": "i <_TFwd>",
    "pcr_tdense_bwd_groups": "i <_TBwd>",
    "pcr_set_stream_min_blocks": "i i",
    "pcr_tdense_fwd_f32": "s <_TFwd>S",
    "pcr_tdense_fwd_pooled": "i <_TFwd>",
    "pcr_tdense_bwd_f32": "s <_TBwd>S",
    "pcr_pack_weight_bf16_dev_f32": "s FiiiiFS",
    "pcr_local_attn_train_fwd_f32": "s FIFiiiiifS",
    "pcr_local_attn_train_bwd_f32": "s FIFFlFiiiiifS",
    "pcr_reduce_parts_f32": "s FiliiiFS",
    "pcr_reduce_multi_f32": "s <_ReduceJob>iS",
    "pcr_bn_fwd_finalize_f32": "s <_BnFwd>S",
    "pcr_bn_bwd_finalize_f32": "s <_BnBwd>S",
    "pcr_sa_l1_fwd_f32": "s FIFFFFFiiiiiS",
    "pcr_sa_l1_bwd_f32": "s FIFFFFFFFiiiiiS",
    "pcr_sa_l1c_fwd_f32": "s FIIFFFFFiiiiiS",
    "pcr_sa_l1c_bwd_f32": "s FIIFFFFFFFiiiiiS",
    "pcr_sa_pool_fwd_f32": "s FFFFIFiiiiS",
    "pcr_sa_pool_bwd_stats_f32": "s FFFFFiiiS",
    "pcr_tnorm_fwd_f32": "s FFFFFFFiiiifiS",
    "pcr_tnorm_bwd_f32": "s FFFFFFFFFiiiiS",
    "pcr_linattn_fwd_f32": "s <_LinAttnP>S",
    "pcr_linattn_bwd_f32": "s <_LinAttnP>S",
    "pcr_attn_tail_ok": "i iiiii",
    "pcr_attn_tail_part_floats": "i iiii",
    "pcr_attn_tail_groups": "i <_AttnTailP>",
    "pcr_attn_tail_fwd_f32": "s <_AttnTailP>S",
    "pcr_attn_tail_bwd_f32": "s <_AttnTailP>S",
    "pcr_attn_head_ok": "i iiiii",
    "pcr_attn_head_part_floats": "i iiiii",
    "pcr_attn_head_groups": "i <_AttnHeadP>",
    "pcr_attn_head_fwd_f32": "s <_AttnHeadP>S",
    "pcr_attn_head_bwd_f32": "s <_AttnHeadP>S",
    "pcr_pool_pair_fwd_f32": "s FFIiiiS",
    "pcr_pool_pair_bwd_f32": "s FIFiiiS",
    "pcr_pool_both_fwd_f32": "s FFIiiiS",
    "pcr_pool_both_bwd_f32": "s FIFiiiS",
    "pcr_channel_max_fwd_f32": "s FFIiiiiS",
    "pcr_channel_max_bwd_f32": "s FIFiiiiS",
    "pcr_bn_sums_f32": "s FFFFifFiFiiiiS",
    "pcr_bn_affine_f32": "s FFFFFFFFifFiiiS",
    "pcr_edge_pool_fwd_f32": "s FFFfFIFiiiiS",
    "pcr_edge_pool_route_f32": "s FFIfFiiiiS",
    "pcr_bmm_apply_f32": "s FFFiiiiS",
    "pcr_bmm_dt_f32": "s FFFiiiS",
    "pcr_pack_weights_multi_f32": "s PiS",
    "pcr_opt_chunk": "i ",
    "pcr_grad_sumsq_f32": "s PIIiPS",
    "pcr_adamw_step_f32": "s PIIiPfFS",
    # C2. auxiliary training losses
    "pcr_kl_pairs_fwd_f32": "s FIFFFFIIiiS",
    "pcr_kl_pairs_bwd_f32": "s FIFFIFFiiS",
    "pcr_triplet_ok": "i ii",
    "pcr_triplet_draw_i32": "s IIIPIIiiS",
    "pcr_pair_dist_f32": "s FFFiiiS",
    "pcr_triplet_select_f32": "s FIIFFFFIIiiS",
    "pcr_pair_dist_bwd_f32": "s FFFFFIFFiiiS",
    # C3. training on a pair list
    "pcr_index_sum_f32": "s FIIFiiiS",
    "pcr_linattn_pairs_ok": "i ii",
    "pcr_linattn_state_fwd_f32": "s FFiFFiiiiS",
    "pcr_linattn_apply_fwd_f32": "s FiFFIIFFiiiiiS",
    "pcr_linattn_apply_bwd_f32": "s FiFFIIFFFFiiiiiS",
    "pcr_linattn_state_bwd_f32": "s FFiFFFiiiiiS",
    # measurement aid
    "pcr_wall_clock_khz": "i ",
    "pcr_last_launch_arith": "i ",
    "pcr_clock_probe": "s PiiS",
}

_RETURN = {"s": ctypes.c_int, "i": ctypes.c_int, "l": ctypes.c_long, "c": ctypes.c_char_p}
_KIND = {"i": ctypes.c_int, "f": ctypes.c_float, "l": ctypes.c_long, "S": ctypes.c_void_p, "P": ctypes.c_void_p,
         "F": FloatPtr, "I": IntPtr}


def kinds(sig):
    """"s FI<SaParams>S" -> ("s", ["F", "I", "<SaParams>", "S"])"""
    ret, _, params = sig.partition(" ")
    out, i = [], 0
    while i < len(params):
        j = params.index(">", i) + 1 if params[i] == "<" else i + 1
        out.append(params[i:j])
        i = j
    return ret, out


def prototype(sig):
    """-> (restype, argtypes) of a SIGNATURES entry"""
    ret, params = kinds(sig)
    return _RETURN[ret], [_KIND[k] if k in _KIND else ctypes.POINTER(globals()[k[1:-1]]) for k in params]
