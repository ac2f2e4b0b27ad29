"""``radargnn_amd.optim.FusedAdam`` (csrc/optim.hip: every parameter in one launch) against ``torch.optim.Adam``.

The oracle is ``torch.optim.Adam`` on the CPU in float64; the yardstick is the same optimizer on the CPU in float32, on identical
inputs.  The bar, everywhere below: the largest absolute error of FusedAdam against the oracle -- over the parameters, over
``exp_avg`` and over ``exp_avg_sq``, each on its own -- is at most 4 x the yardstick's error on the same quantity (the factor allows
another valid order of the roundings of one element's update).  The yardstick's error is computed here, next to the comparison."""
import copy
import math

import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, 4099]
VIEW_LEN = 1027                       # one further parameter: a view one float into its storage
QUANTITIES = ("p", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def FusedAdam():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd.optim import FusedAdam
    return FusedAdam


def make_inputs(sizes, steps, seed):
    """initial values N(0, 1) and per-step gradients N(0, 1) * 10^((i mod 5) - 2) for tensor i, float32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * 10.0 ** ((i % 5) - 2) for i, n in enumerate(sizes)] for _ in range(steps)]
    return init, grads


def run_torch(init, grads, dtype, device="cpu", skip=(), scheduler=None, **hyper):
    """torch.optim.Adam over the steps; ``skip``: (step, tensor) pairs whose gradient is None"""
    params = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in init]
    opt = torch.optim.Adam(params, **hyper)
    sched = scheduler(opt) if scheduler else None
    for s, step_grads in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, step_grads)):
            p.grad = None if (s, i) in skip else g.to(device=device, dtype=dtype)
        opt.step()
        if sched:
            sched.step()
    return params, opt


def device_params(init, view_last=False):
    """float32 parameters on the GPU; with ``view_last`` the last one is a view at a storage offset of one float"""
    params = [torch.nn.Parameter(p.cuda()) for p in init]
    if view_last:
        base = torch.zeros(init[-1].numel() + 1, device="cuda")
        base[1:].copy_(init[-1])
        params[-1] = torch.nn.Parameter(base[1:])
        assert params[-1].storage_offset() == 1 and params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    return params


def run_fused(FusedAdam, params, grads, skip=(), scheduler=None, **hyper):
    """FusedAdam over the steps.  Every gradient is a NEW tensor: the previous step's gradients are kept alive and an unrelated
    allocation is made in between, so no address of one step is an address of the next."""
    opt = FusedAdam(params, **hyper)
    sched = scheduler(opt) if scheduler else None
    keep, seen = [], set()
    for s, step_grads in enumerate(grads):
        fresh = []
        for i, (p, g) in enumerate(zip(params, step_grads)):
            keep.append(torch.empty(1000 + 37 * (s + i), device="cuda"))
            p.grad = None if (s, i) in skip else g.cuda()
            if p.grad is not None:
                fresh.append(p.grad)
                assert p.grad.data_ptr() not in seen
                seen.add(p.grad.data_ptr())
        opt.step()
        keep.extend(fresh)
        if sched:
            sched.step()
    return opt


def collect(params, opt):
    def state(p, key):
        st = opt.state.get(p)
        return st[key].detach().double().cpu() if st else torch.zeros_like(p).double().cpu()
    return {"p": [p.detach().double().cpu() for p in params], "exp_avg": [state(p, "exp_avg") for p in params],
            "exp_avg_sq": [state(p, "exp_avg_sq") for p in params]}


def max_errors(got, oracle):
    return {q: max(float((a - b).abs().max()) for a, b in zip(got[q], oracle[q])) for q in QUANTITIES}


def assert_within_bar(name, fused, yardstick, oracle):
    ef, ey = max_errors(fused, oracle), max_errors(yardstick, oracle)
    ratio = {q: (ef[q] / ey[q] if ey[q] > 0 else (0.0 if ef[q] == 0 else math.inf)) for q in QUANTITIES}
    record_parity(name, **{f"{q}_err_over_f32_adam": ratio[q] for q in QUANTITIES}, **{f"{q}_f32_adam_err": ey[q] for q in QUANTITIES})
    for q in QUANTITIES:
        assert ef[q] <= 4.0 * ey[q], f"{q}: FusedAdam {ef[q]:.3e} vs float64, float32 torch.optim.Adam {ey[q]:.3e} (x{ratio[q]:.2f})"


@pytest.mark.parametrize("weight_decay", [1e-4, 0.0])
def test_parity_with_float64_adam(FusedAdam, weight_decay):
    init, grads = make_inputs(SIZES + [VIEW_LEN], steps=10, seed=11)
    hyper = dict(lr=1e-3, weight_decay=weight_decay)
    oracle = collect(*run_torch(init, grads, torch.float64, **hyper))
    yardstick = collect(*run_torch(init, grads, torch.float32, **hyper))
    params = device_params(init, view_last=True)
    opt = run_fused(FusedAdam, params, grads, **hyper)
    assert opt.launches_last_step == 1                      # ten tensors: one launch
    assert all(opt.state[p]["step"] == 10 for p in params)
    assert_within_bar(f"fused_adam_wd{weight_decay:g}", collect(params, opt), yardstick, oracle)


def test_per_tensor_steps_follow_missing_gradients(FusedAdam):
    """a parameter without a gradient is skipped: no moment decay, no step increment (torch keeps ``state['step']`` per parameter)"""
    init, grads = make_inputs([65, 257, 1025], steps=5, seed=12)
    skip = {(1, 1), (2, 1)}                                  # tensor 1 has no gradient in steps 2 and 3 of 5
    hyper = dict(lr=1e-3, weight_decay=1e-4)
    ref_params, ref_opt = run_torch(init, grads, torch.float64, skip=skip, **hyper)
    assert float(ref_opt.state[ref_params[1]]["step"]) == 3
    oracle = collect(ref_params, ref_opt)
    yardstick = collect(*run_torch(init, grads, torch.float32, skip=skip, **hyper))
    params = device_params(init)
    opt = run_fused(FusedAdam, params, grads, skip=skip, **hyper)
    assert [opt.state[p]["step"] for p in params] == [5, 3, 5]
    assert_within_bar("fused_adam_skipped_steps", collect(params, opt), yardstick, oracle)
    only = lambda run: {q: [run[q][1]] for q in QUANTITIES}  # and the skipped tensor on its own
    assert_within_bar("fused_adam_skipped_tensor", only(collect(params, opt)), only(yardstick), only(oracle))


def small_model(seed=0):
    from radargnn_amd import gnn
    cfg = gnn.GNNArchitectureConfig(node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=[16, 8],
                                    classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[8, 5],
                                    initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
                                    node_feature_embedding_layer_dimensions=[8, 16], edge_feature_embedding_layer_dimensions=[4, 8],
                                    conv_layer_type="MPNNConv", batch_norm_in_mlps=False)
    torch.manual_seed(seed)
    return gnn.DetNetBasic(cfg).cuda(), cfg


def test_weight_caches_follow_the_update(FusedAdam):
    """The kernel writes parameters through raw pointers; the package's weight-derived caches are keyed on ``Tensor._version``.
    After a step, a forward must use the NEW weights: bit for bit what a fresh model built from the state dict computes."""
    from radargnn_amd import gnn
    model, cfg = small_model()
    g = torch.Generator().manual_seed(1)
    n, e = 2400, 14400
    x = torch.randn(n, 5, generator=g).cuda(); ei = torch.randint(0, n, (2, e), generator=g).cuda()
    ea = torch.randn(e, 2, generator=g).cuda()
    label = torch.randint(0, 6, (n,), generator=g).float().view(-1, 1)
    y = torch.cat((label, torch.randn(n, 5, generator=g)), 1).cuda()
    with torch.no_grad():
        before = model(x, ei, ea)                           # fills the caches of the inference path
    c, b = model(x, ei, ea)                                 # ... and of the training path
    loss, _, _ = gnn.detection_loss(c, b, y, 5)
    loss.backward()
    params = [p for p in model.parameters() if p.grad is not None]
    assert params
    versions = [p._version for p in params]
    FusedAdam(model.parameters(), lr=1e-2).step()
    assert all(p._version > v for p, v in zip(params, versions))
    with torch.no_grad():
        after = model(x, ei, ea)
        fresh = gnn.DetNetBasic(cfg).cuda()
        fresh.load_state_dict(model.state_dict())
        expect = fresh(x, ei, ea)
    assert not torch.equal(after[0], before[0])             # the step moved the weights
    assert torch.equal(after[0], expect[0]) and torch.equal(after[1], expect[1])


def test_more_tensors_than_one_launch_holds(FusedAdam):
    from radargnn_amd import ops
    capacity = ops.adam_capacity()
    assert capacity >= 64
    count = 300
    init, grads = make_inputs([3] * count, steps=3, seed=13)
    hyper = dict(lr=1e-3, weight_decay=1e-4)
    oracle = collect(*run_torch(init, grads, torch.float64, **hyper))
    yardstick = collect(*run_torch(init, grads, torch.float32, **hyper))
    flat = torch.cat(init).cuda()                           # views 3 floats apart: every alignment, tensors shorter than a float4
    params = [torch.nn.Parameter(flat[3 * i:3 * i + 3]) for i in range(count)]
    assert {p.data_ptr() % 16 for p in params} == {0, 4, 8, 12}
    opt = run_fused(FusedAdam, params, grads, **hyper)
    assert opt.launches_last_step == math.ceil(count / capacity)
    assert_within_bar("fused_adam_300_tensors", collect(params, opt), yardstick, oracle)


def test_scheduler_drives_the_learning_rate(FusedAdam):
    init, grads = make_inputs([65, 257, 1025], steps=3, seed=14)
    hyper = dict(lr=1e-2, weight_decay=1e-4)
    sched = lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    oracle = collect(*run_torch(init, grads, torch.float64, scheduler=sched, **hyper))
    yardstick = collect(*run_torch(init, grads, torch.float32, scheduler=sched, **hyper))
    params = device_params(init)
    opt = run_fused(FusedAdam, params, grads, scheduler=sched, **hyper)
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-2 * 0.5 ** 3)
    assert_within_bar("fused_adam_exponential_lr", collect(params, opt), yardstick, oracle)


def test_state_dict_round_trips_with_torch_adam(FusedAdam):
    """three steps with one optimizer, its state dict loaded into the other, two more steps: the parameters continue as the
    oracle's five uninterrupted steps do, in both directions"""
    init, grads = make_inputs([65, 257, 1025], steps=5, seed=15)
    hyper = dict(lr=1e-3, weight_decay=1e-4)
    oracle = collect(*run_torch(init, grads, torch.float64, **hyper))
    yardstick = collect(*run_torch(init, grads, torch.float32, **hyper))

    def continue_with(make_opt, params, saved):
        opt = make_opt(params, **hyper)
        opt.load_state_dict(copy.deepcopy(saved))
        for step_grads in grads[3:]:
            for p, g in zip(params, step_grads):
                p.grad = g.cuda()
            opt.step()
        return opt

    params = device_params(init)                            # FusedAdam -> torch.optim.Adam
    first = run_fused(FusedAdam, params, grads[:3], **hyper)
    saved = first.state_dict()
    assert set(saved["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and saved["state"][0]["step"] == 3
    opt = continue_with(torch.optim.Adam, params, saved)
    assert all(float(opt.state[p]["step"]) == 5 for p in params)
    assert_within_bar("fused_adam_state_into_torch", collect(params, opt), yardstick, oracle)

    params, first = run_torch(init, grads[:3], torch.float32, device="cuda", **hyper)   # torch.optim.Adam -> FusedAdam
    opt = continue_with(FusedAdam, params, first.state_dict())
    assert all(opt.state[p]["step"] == 5 for p in params)
    assert_within_bar("torch_state_into_fused_adam", collect(params, opt), yardstick, oracle)


def test_unsupported_flags_and_tensors_raise(FusedAdam):
    p = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    for flag in ("amsgrad", "maximize", "decoupled_weight_decay", "capturable", "differentiable"):
        with pytest.raises(ValueError):
            FusedAdam([p], **{flag: True})
    before = p.detach().clone()
    for bad, grad in ((torch.zeros(8, device="cuda", dtype=torch.float64), torch.ones(8, device="cuda", dtype=torch.float64)),
                      (torch.zeros(8, 2, device="cuda")[:, 0], torch.ones(8, device="cuda")),          # not contiguous
                      (torch.zeros(8), torch.ones(8))):                                                # on the CPU
        q = torch.nn.Parameter(bad)
        opt = FusedAdam([p, q])
        p.grad = torch.ones(8, device="cuda"); q.grad = grad
        with pytest.raises(TypeError):
            opt.step()
        assert torch.equal(p, before) and not opt.state[p]  # refused before anything was launched or counted
