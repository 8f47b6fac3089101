"""CPU: the float64 restatement behind the PointNet++ SSG training tests (tests/ssg_train_ref.py) is tied to the pinned
oracle, its planted faults show at the bounds the GPU tests use on the very inputs they use, those inputs condition to
zero marginal float64 decisions within MOVE_CAP; the new symbols, their bad-argument statuses and the module's refusals
come back without a device."""
import numpy as np
import pytest
import torch

import ssg_train_ref as G

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _sd64(sd):
    return {k: (v.to(F64) if v.is_floating_point() else v) for k, v in sd.items()}


# ----------------------------------------------------------------------------- ties to the pinned oracle --
@pytest.mark.parametrize("i", range(len(G.MODULE_CASES)))
def test_restatement_with_running_statistics_is_the_oracles_layer(i):
    """BatchNorm switched to the running statistics, the scale is model_oracle.ssg_sa_layer (pinned by test_gpu_ssg.py)
    to 1e-12 in float64, centres and indices from the same C oracle"""
    import model_oracle as MO
    c, case = G.MODULE_CASES[i], G.module_case(i)
    sd = _sd64(case["sd"])
    xyz = case["xyz"].to(F64)
    feats = None if case["feats"] is None else case["feats"].to(F64)
    r = G.scale_ref(G.layers_of(case["sd"]), xyz, feats, case["idx"], case["centre"], running=True)
    new_xyz, want = MO.ssg_sa_layer(sd, xyz, feats, c["S"], c["r"], c["K"])
    assert want.dtype == F64 and _rel(r["out"], want) < 1e-12
    assert torch.equal(new_xyz, torch.gather(xyz, 1, case["centre"].long().unsqueeze(2).expand(-1, -1, 3)))


@pytest.mark.parametrize("i", range(len(G.MODULE_CASES)))
def test_table_form_is_the_gathered_first_conv(i):
    case = G.module_case(i)
    p = G.layers_of(case["sd"])[0]
    xyz = case["xyz"].to(F64)
    feats = None if case["feats"] is None else case["feats"].to(F64)
    idx, centre = case["idx"], case["centre"]
    B, S, K = idx.shape
    want = torch.einsum("oc,bcsk->bosk", p["W"], G.group_rows(xyz, feats, idx, centre)).reshape(B, -1, S * K)
    tab = None if feats is None else torch.einsum("oc,bcn->bon", p["W"][:, 3:], feats)
    got = G.sa_l1c_ref(xyz, idx, centre, tab, p["W"][:, :3].contiguous(), None)
    assert _rel(got, want) < 1e-12


def test_first_argmax_gather_routes_a_tie_between_copies_to_slot_zero():
    case = G.module_case(0)
    r = G.scale_ref(G.layers_of(case["sd"]), case["xyz"].to(F64), None, case["idx"], case["centre"])
    cnt = G.genuine_count(case["idx"]).unsqueeze(1).expand_as(r["arg"])
    assert bool((r["arg"] < cnt).all())                   # a copy never wins: its row 0 comes first
    assert bool(((r["arg"] == 0) & (cnt < case["idx"].shape[2]) & (r["out"] > 0)).any())      # and row 0 does win somewhere


# ------------------------------------------------------------------------------------------ conditioning --
@pytest.mark.parametrize("i", range(len(G.MODULE_CASES)))
def test_module_inputs_condition_within_the_cap(i):
    c, case = G.MODULE_CASES[i], G.module_case(i)
    print(dict(case=i, moved=case["moved"], total=case["total"]))
    assert case["moved"] <= G.MOVE_CAP * case["total"], (case["moved"], case["total"])
    assert G.count_marginals(G.layers_of(case["sd"]), case["xyz"], case["feats"], case["idx"], case["centre"]) == 0
    centre, idx = G.oracle_query(c["S"], c["r"], c["K"])(case["xyz"])
    assert torch.equal(centre, case["centre"]) and torch.equal(idx, case["idx"])
    cnt = G.genuine_count(idx)
    assert bool((cnt < c["K"]).any())                     # copies are present
    if c["kind"] == "dup":                                # the conditioned cloud keeps its exact duplicates
        assert all(len(torch.unique(cloud, dim=0)) < c["N"] for cloud in case["xyz"])
        assert int(centre.max()) >= c["S"]


def test_ball_index_sets_of_the_launch_cases_hold_copies_and_lone_centres():
    for shape in G.L1C_SHAPES:
        B, N, S, K, c1 = shape
        inp = G.make_l1c_input(shape, "ball", True, False, G.oracle_query(S, G.BALL_RADIUS, K))
        cnt = G.genuine_count(inp["idx"])
        if K > 1:
            assert bool((cnt < K).any()) and bool((cnt == 1).any()), shape
    perm = G.make_l1c_input(G.L1C_SHAPES[0], "random", True, True)["centre"]
    assert int(perm[0].min()) >= G.L1C_SHAPES[0][2]       # every centre index >= S in cloud 0
    assert all(len(set(row.tolist())) == perm.shape[1] for row in perm)


# ------------------------------------------------------------------------------------- planted faults --
def _bound(i):
    return G.BF_BOUND if G.MODULE_CASES[i]["mlp"][1:3] == [128, 128] else G.BN_BOUND


@pytest.mark.parametrize("i,fault", [(i, f) for i in range(len(G.MODULE_CASES)) for f in G.FAULTS
                                     if not (f == "dtab_without_copies" and G.MODULE_CASES[i]["mlp"][0] == 0)])
def test_planted_fault_shows_at_the_gpu_bound(i, fault):
    """each wrong reading of the issue moves at least one compared output beyond the bound of the GPU module test"""
    case = G.module_case(i)
    args = (case["sd"], case["xyz"], case["feats"], case["idx"], case["centre"], case["w"])
    good, bad = G.scale_outputs(*args), G.scale_outputs(*args, fault=fault)
    moved = {k: _rel(bad[k].to(F64), good[k].to(F64)) for k in good if k != "arg"}
    print(dict(case=i, fault=fault, worst=max(moved, key=moved.get), rel=max(moved.values())))
    assert max(moved.values()) > _bound(i), moved
    if fault == "dtab_without_copies":
        assert moved["grad:feats"] > _bound(i)


# --------------------------------------------------------------------------------- symbols and statuses --
@pytest.fixture(scope="module")
def lib():
    from pcr_amd import _lib, build
    build.build()
    return _lib.load()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    from pcr_amd import abi
    for name in ("pcr_sa_l1c_fwd_f32", "pcr_sa_l1c_bwd_f32"):
        assert hasattr(lib, name) and name in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17


def test_bad_arguments_return_a_status_without_a_device(lib):
    """NULL centre, N beyond the LDS rule (one channel's table row in 32 KiB: N <= 8192), K or S <= 0: PCR_ERR_INVALID
    before anything touches the device (the pointers here are host addresses: a launch would fault)"""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def fwd(centre=p, B=1, N=16, S=4, K=2, c1=4):
        return lib.pcr_sa_l1c_fwd_f32(p, p, centre, None, p, None, p, None, B, N, S, K, c1, None)

    def bwd(centre=p, B=1, N=16, S=4, K=2, c1=4):
        return lib.pcr_sa_l1c_bwd_f32(p, p, centre, p, p, p, p, p, None, p, B, N, S, K, c1, None)
    for f in (fwd, bwd):
        assert f(centre=None) == 1
        assert f(N=8193) == 1 and f(N=1 << 20) == 1
        assert f(K=0) == 1 and f(K=-3) == 1 and f(S=0) == 1 and f(S=-1) == 1
        assert f(c1=0) == 1 and f(B=-1) == 1 and f(B=70000) == 1
        assert f(B=0) == 0                                # an empty batch is fine and launches nothing
    assert lib.pcr_sa_l1c_fwd_f32(None, p, p, None, p, None, p, None, 1, 16, 4, 2, 4, None) == 1
    # the existing pair keeps its rule (centres are the first S points: S <= N)
    assert lib.pcr_sa_l1_fwd_f32(p, p, None, p, p, p, None, 1, 16, 17, 2, 4, None) == 1


# ------------------------------------------------------------------------------------------- refusals --
def _sa(**kw):
    from mmdet3d.ops.pointnet_modules import PointSAModule
    args = dict(mlp_channels=[4, 8, 8, 8], num_point=4, radius=0.5, num_sample=4)
    args.update(kw)
    m = PointSAModule(**args)
    m.hip_training = True
    return m.train()


def _variants():
    from mmdet3d.ops.pointnet_modules import GroupAll, PointSAModuleMSG
    msg = PointSAModuleMSG(num_point=4, radii=[0.2, 0.4], sample_nums=[4, 4], mlp_channels=[[4, 8, 8, 8], [4, 8, 8, 8]])
    dil = PointSAModuleMSG(num_point=4, radii=[0.4], sample_nums=[4], mlp_channels=[[4, 8, 8, 8]], dilated_group=True)
    for m in (msg, dil):
        m.hip_training = True
        m.train()
    ga = _sa()
    ga.groupers[0] = GroupAll()
    mom = _sa()
    mom.mlps[0].layer1.bn.momentum = None
    act, norm = _sa(), _sa()
    act.mlps[0].layer2.activate = None                    # a ConvModule without its ReLU, one without its BatchNorm
    norm.mlps[0].layer0.bn = torch.nn.Identity()
    return dict(msg=msg, dilated_group=dil, avg=_sa(pool_mod="avg"), normalize_xyz=_sa(normalize_xyz=True),
                no_xyz=_sa(use_xyz=False), two_layers=_sa(mlp_channels=[4, 8, 8]), four_layers=_sa(mlp_channels=[4, 8, 8, 8, 8]),
                group_all=ga, momentum_none=mom, no_relu=act, no_norm=norm)


def test_refusals_under_the_switch_raise_before_any_launch(monkeypatch):
    from pcr_amd import _lib
    launched = []
    real = _lib.load
    monkeypatch.setattr(_lib, "load", lambda: launched.append(1) or real())
    xyz, feats = torch.randn(2, 16, 3), torch.randn(2, 4, 16)         # host tensors: any launch would be refused, differently
    variants = _variants()
    assert len(variants) == 11
    for name, m in variants.items():
        with pytest.raises(_lib.PcrError, match="HIP training graph covers"):
            m(xyz, feats)
    assert not launched
    assert _sa()._training_refusal() is None


def test_default_module_and_model_refuse_train_mode_as_before():
    from mmdet3d.models.pointnet2_ssg import PointNet2SSG
    from mmdet3d.ops.pointnet_modules import PointSAModule
    from pcr_amd import _lib
    m = PointSAModule(mlp_channels=[4, 8, 8, 8], num_point=4, radius=0.5, num_sample=4)
    assert m.hip_training is False
    m.train()
    with pytest.raises(_lib.PcrError, match="eval-mode inference; call .eval\\(\\)"):
        m._plan(0, torch.device("cpu"))
    with pytest.raises(_lib.PcrError, match="eval-mode inference; call .eval\\(\\)"):
        m(torch.randn(2, 16, 3), torch.randn(2, 4, 16))
    net = PointNet2SSG(num_points=(8, 4), radii=(0.4, 0.8), num_samples=(4, 4), sa_channels=((8, 8, 8), (8, 8, 8)))
    assert not net.trainable and not any(sa.hip_training for sa in net.SA_modules)
    net.train()
    with pytest.raises(_lib.PcrError, match="eval-mode inference; call .eval\\(\\)"):
        net(torch.randn(2, 16, 3))
    on = PointNet2SSG(num_points=(8, 4), radii=(0.4, 0.8), num_samples=(4, 4), sa_channels=((8, 8, 8), (8, 8, 8)), trainable=True)
    assert on.trainable and all(sa.hip_training for sa in on.SA_modules)
    assert sorted(on.state_dict()) == sorted(net.state_dict())       # the switch adds no parameter or buffer


def test_whole_step_restatement_runs_in_both_precisions():
    """the float64 and float32 restatements of the model test's step agree to float32 rounding (the float32 one is the
    yardstick of the GPU test's rule); every parameter gets a gradient"""
    cfg = dict(G.MODEL_BACKBONE)
    sd = model_state_dict()
    s1, s2, match = model_inputs()
    q = G.oracle_query
    l64, g64, _, _ = G.step_ref(sd, s1, s2, match, cfg, q, F64)
    l32, g32, _, _ = G.step_ref(sd, s1, s2, match, cfg, q, torch.float32)
    assert abs(float(l64) - float(l32)) < 1e-5
    params = [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    assert sorted(g64) == sorted(params) == sorted(g32)


def model_cfg():
    import copy
    import bench
    cfg = copy.deepcopy(bench.SSG_MODEL)
    cfg["backbone"] = dict(G.MODEL_BACKBONE)
    return cfg


def model_state_dict():
    from mmdet3d.models import build_model
    from pcr_amd import testing as T
    m = build_model(model_cfg())
    return T.seeded_state_dict(T.manifest_of(m), 0)


def model_inputs():
    from pcr_amd import testing as T
    s1, s2 = T.synthetic_pairs(G.MODEL_PAIRS, G.MODEL_N, seed=9, kind="dup")
    ids1 = torch.arange(G.MODEL_PAIRS)
    ids2 = torch.where(ids1 < G.MODEL_PAIRS // 2, ids1, ids1 + 100)
    return s1, s2, (ids1 == ids2).float()
