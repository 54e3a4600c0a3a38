"""The generator's weight average on the GPU: pg_adam_ema / pg_adam_dev_ema against pg_adam /
pg_adam_dev (parameters and moments bitwise, the average against the float64 formula), the
average inside the training step in its eager, C++-replayed and hipGraph forms, training left
bit for bit as it is without it, the carry-over through a stage change, and sampling.

The one-step bound (assert_one_step, derived in tests/test_ema_cpu.py): 8 * 2^-24 *
max(|ema_prev|, |p_new|) per element."""
import pytest
import torch

from gen_inputs import TINY_DEPTHS
from test_ema_cpu import assert_one_step, live_dead
from test_gpu_graph import build
from test_model_api import make_args

pytestmark = pytest.mark.gpu

N_LOOP = 4194304 + 48      # just past grid_for's 16384 blocks x 256 threads: the stride loop loops


# ------------------------------------------------------------------ op level
@pytest.fixture(scope="module")
def op_inputs():
    """p, g (two steps), m, v, ema at the largest size with 64 spare elements, drawn once and
    left unchanged; every case slices its own n + 64."""
    gen = torch.Generator(device="cuda").manual_seed(3)
    r = lambda: torch.randn(N_LOOP + 64, device="cuda", generator=gen)
    return dict(p=r(), g1=r(), g2=r() * 1e-3, m=r() * 0.1, v=r().square() * 0.1, ema=r())


@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("beta1", [0.0, 0.5])
@pytest.mark.parametrize("n", [16, 10000, N_LOOP])
def test_ops_match_adam_and_formula(op_inputs, n, beta1, decay):
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.float32)
    kw = dict(lr=1e-3, beta1=beta1, beta2=0.99, eps=1e-8)
    src = {k: t[:n + 64] for k, t in op_inputs.items()}
    for dev in (False, True):
        a = {k: src[k].clone() for k in ("p", "m", "v")}                # plain entry
        b = {k: src[k].clone() for k in ("p", "m", "v", "ema")}         # fused entry
        sa, sb = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        for t, g in enumerate((src["g1"], src["g2"]), start=1):
            prev = b["ema"].clone()
            if dev:
                ops.adam_dev(a["p"][:n], g[:n], a["m"][:n], a["v"][:n], step_dev=sa, **kw)
                ops.adam_dev_ema(b["p"][:n], g[:n], b["m"][:n], b["v"][:n], b["ema"][:n],
                                 decay=decay, step_dev=sb, **kw)
            else:
                ops.adam(a["p"][:n], g[:n], a["m"][:n], a["v"][:n], step=t, **kw)
                ops.adam_ema(b["p"][:n], g[:n], b["m"][:n], b["v"][:n], b["ema"][:n],
                             decay=decay, step=t, **kw)
            torch.cuda.synchronize()
            for k in ("p", "m", "v"):
                assert torch.equal(a[k], b[k]), (dev, t, k)
            assert not torch.equal(b["p"][:n], src["p"][:n])
            assert_one_step(b["ema"][:n], prev[:n], b["p"][:n], decay, (dev, t))
            for k in ("p", "m", "v", "ema"):                             # beyond n: untouched
                assert torch.equal(b[k][n:], src[k][n:]), (dev, t, k)
        if dev:
            assert int(sa.item()) == int(sb.item()) == 2


def test_ops_reject_bad_arguments():
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.float32)
    t = [torch.zeros(16, device="cuda") for _ in range(5)]
    sd = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(lr=1e-3, beta1=0.0, beta2=0.99, eps=1e-8)
    with pytest.raises(RuntimeError, match="adam_ema"):
        ops.adam_ema(*t[:4], None, decay=0.5, step=1, **kw)
    with pytest.raises(RuntimeError, match="adam_dev_ema"):
        ops.adam_dev_ema(*t[:4], None, decay=0.5, step_dev=sd, **kw)
    for decay in (1.0, 1.5, -0.5, float("nan")):      # 1 - decay outside (0, 1]
        with pytest.raises(RuntimeError, match="one_minus_decay"):
            ops.adam_ema(*t, decay=decay, step=1, **kw)
        with pytest.raises(RuntimeError, match="one_minus_decay"):
            ops.adam_dev_ema(*t, decay=decay, step_dev=sd, **kw)
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in t) and int(sd.item()) == 0


# ------------------------------------------------------------------ step level
def model(tmp_path, s, dtype="f32", decay=0.5, replay=False, graph=False):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), compute_dtype=dtype, ema_decay=decay)
    m = build(args, graph, s)
    m.use_replay = replay
    m.G.alpha = m.D.alpha = 0.5
    return m


def test_eager_step_follows_the_recursion(tmp_path):
    m = model(tmp_path, 2)
    assert torch.equal(m.fpG.ema, m.fpG.flat) and m.fpD.ema is None
    live, dead = live_dead(m.fpG)
    assert dead == ["toRGB_blocks.0.toRGB.module.bias", "toRGB_blocks.0.toRGB.module.weight"]
    params = dict(m.G_ema.named_parameters())
    for step in range(3):
        prev = {n: p.detach().clone() for n, p in params.items()}
        m.train_step()
        torch.cuda.synchronize()
        for n in live:
            assert params[n].data_ptr() == m.fpG.eviews[n].data_ptr()
            assert_one_step(params[n], prev[n], m.fpG.views[n], 0.5, (step, n))
            if n.endswith("weight"):
                assert not torch.equal(params[n], prev[n]), (step, n)
        for n in dead:
            assert torch.equal(params[n], prev[n]), (step, n)
    assert m.graph_replays == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_not_perturbed(tmp_path, dtype):
    off, on = model(tmp_path, 2, dtype, decay=None), model(tmp_path, 2, dtype, decay=0.5)
    assert off.G_ema is None and off.fpG.ema is None
    for step in range(3):
        off.train_step()
        on.train_step()
        torch.cuda.synchronize()
        for net in ("fpG", "fpD"):
            for buf in ("flat", "m", "v"):
                assert torch.equal(getattr(getattr(off, net), buf),
                                   getattr(getattr(on, net), buf)), (step, net, buf)
        lo, ln = (next(iter(x._engines.values())).loss for x in (off, on))
        assert torch.equal(lo, ln), step
    assert not torch.equal(on.fpG.ema, on.fpG.flat)


@pytest.mark.parametrize("form", ["replay", "graph"])
def test_replayed_forms_match_eager(tmp_path, form):
    eager = model(tmp_path, 2)
    rep = model(tmp_path, 2, replay=form == "replay", graph=form == "graph")
    for step in range(6):
        eager.train_step()
        rep.train_step()
        torch.cuda.synchronize()
        assert torch.equal(eager.fpG.ema, rep.fpG.ema), step
        assert torch.equal(eager.fpG.flat, rep.fpG.flat), step
    assert rep.graph_replays > 0 and eager.graph_replays == 0
    assert not torch.equal(rep.fpG.ema, rep.fpG.flat)
    if form == "replay":
        # the average adds no launch: the recorded step is as long as without it
        off = model(tmp_path, 2, decay=None, replay=True)
        for _ in range(3):
            off.train_step()
        torch.cuda.synchronize()
        n_on, n_off = len(rep._gstate["rec"]), len(off._gstate["rec"])
        assert n_on == n_off and n_on > 50, (n_on, n_off)


def test_stage_change_carries_the_average_by_name(tmp_path):
    m = model(tmp_path, 1)
    for _ in range(2):
        m.train_step()
    torch.cuda.synchronize()
    old = {n: v.clone() for n, v in m.fpG.eviews.items()}
    assert any(not torch.equal(old[n], m.fpG.views[n]) for n in old)
    m.change_scale(2)
    new = [n for n in m.fpG.names if n not in old]
    assert len(new) == 6 and len(m.G_ema.blocks) == len(m.G.blocks) == 2
    for n in old:
        assert torch.equal(m.fpG.eviews[n], old[n]), n
    for n in new:
        assert torch.equal(m.fpG.eviews[n], m.fpG.views[n]), n
    for n, p in m.G_ema.named_parameters():
        assert p.data_ptr() == m.fpG.eviews[n].data_ptr(), n
    before = {n: m.fpG.eviews[n].clone() for n in new}
    m.G.alpha = m.D.alpha = 0.5        # at alpha 0 the new block gets no gradient yet
    m.train_step()
    torch.cuda.synchronize()
    for n in new:
        assert not torch.equal(m.fpG.eviews[n], before[n]), n
        assert_one_step(m.fpG.eviews[n], before[n], m.fpG.views[n], 0.5, n)


def test_sampling(tmp_path):
    from pggan_amd import nets
    m = model(tmp_path, 2)
    m.train_step()
    z = torch.randn(4, m.args.latent_dim, device="cuda",
                    generator=torch.Generator(device="cuda").manual_seed(5))
    img = m.sample(z)
    assert img.shape == (4, 3, 16, 16) and m.G_ema.alpha == m.G.alpha == 0.5
    fresh = nets.Generator(m.args.latent_dim, TINY_DEPTHS[0]).to("cuda")
    for i in (1, 2):
        fresh.add_block(TINY_DEPTHS[i])
    fresh.load_state_dict(m.G_ema.state_dict())
    fresh.alpha = m.G.alpha
    with torch.no_grad():
        ref = fresh(z)
    assert torch.equal(img, ref)
    assert not torch.equal(img, m.sample(z, ema=False))
    with torch.no_grad():
        assert torch.equal(m.sample(z, ema=False), m.G(z))

    off = model(tmp_path, 2, decay=None)
    assert off.G_ema is None and off.fpG.ema is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.sample(z)
    assert off.sample(z, ema=False).shape == (4, 3, 16, 16)
