"""The generator's weight average (config `ema_decay`, ProgressiveGAN.G_ema) on the CPU test
double (tests/cpu_ops.py has no fused Adam+EMA entry, so StepEngine.adam runs the plain update
followed by the recursion): the recursion itself, dead parameters frozen, the carry-over by
name through change_scale, the G_ema_*.pt checkpoint files beside the reference's unchanged
ones, and two gloo ranks with the deferred generator update.

The one-step bound used here and in tests/test_gpu_ema.py: ema' = ema + c (p - ema) in fp32 is
three roundings, the worst on p - ema <= 2 max(|ema|, |p|), so the result is within
5 * 2^-24 * max(|ema|, |p|) of the float64 value with or without multiply-add contraction;
8 leaves margin without hiding a wrong coefficient (decay 0.5 against 0.999 differs by half
the distance between ema and p)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gen_inputs import TINY_DEPTHS, make_inputs, make_params

from cpu_ops import CpuOps
from pggan_amd import _lib
from pggan_amd import nets
from pggan_amd.model import ProgressiveGAN
from test_dp_gloo import _free_port
from test_model_api import fresh_model, make_args

SCHED = dict(max_step_at_scale=[2, 5, 5], alpha_jump_start=[-1, 0, 0],
             alpha_jump_interval=[0, 1, 1], alpha_jump_Ntimes=[0, 4, 4])


@pytest.fixture(autouse=True)
def _cpu_ops(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(CpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOps)
    nets._ENGINES.clear()


def assert_one_step(ema_new, ema_prev, p_new, decay, what=""):
    """ema_new is one update of ema_prev towards p_new, elementwise, within the bound above."""
    c = _lib.one_minus_decay(decay)
    e0, p = ema_prev.detach().double(), p_new.detach().double()
    want = e0 + c * (p - e0)
    bound = 8 * 2.0 ** -24 * torch.maximum(e0.abs(), p.abs())
    err = (ema_new.detach().double() - want).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float(bound.max()))


def live_dead(fp):
    live = [n for n in fp.names if n not in fp.dead]
    return live, sorted(fp.dead)


def test_off_by_default(tmp_path):
    m = fresh_model(make_args(tmp_path))
    assert m.hyper.ema_decay == 0.0 and m.G_ema is None and m.fpG.ema is None
    m.train_step()
    with pytest.raises(RuntimeError, match="ema_decay"):
        m.sample(torch.zeros(2, m.args.latent_dim))
    assert m.sample(torch.zeros(2, m.args.latent_dim), ema=False).shape == (2, 3, 4, 4)
    with pytest.raises(ValueError):
        ProgressiveGAN(make_args(tmp_path, ema_decay=1.0), "cpu")


def test_entry_points_reject_bad_arguments():
    """pg_adam_ema / pg_adam_dev_ema refuse a null `ema` and a coefficient outside (0, 1] on
    the host, before any launch (the pointers here are never dereferenced)."""
    import ctypes
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    lib = _lib.load_library()
    buf = (ctypes.c_float * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    step = ctypes.cast((ctypes.c_int * 1)(), ctypes.c_void_p)
    assert _lib.one_minus_decay(0.999) == ctypes.c_float(1.0 - 0.999).value != 1.0 - 0.999
    for omd, ema in ((0.5, None), (0.0, ptr), (-0.5, ptr), (1.5, ptr), (float("nan"), ptr)):
        assert lib.pg_adam_ema(16, ptr, ptr, ptr, ptr, ema, omd, 1e-3, 0.0, 0.99, 1e-8, 1,
                               None) != 0, (omd, ema)
        assert b"adam_ema" in lib.pg_last_error()
        assert lib.pg_adam_dev_ema(16, ptr, ptr, ptr, ptr, ema, omd, 0.0, 0.99, 1e-8, ptr, 1,
                                   step, None) != 0, (omd, ema)
        assert b"adam_dev_ema" in lib.pg_last_error()


def test_fallback_path_gives_the_recursion(tmp_path):
    """Three steps at stage 2 (toRGB_blocks.0 dead): live names follow the recursion over the
    post-step G, dead names and D are left alone, G_ema is the reference-shaped view of it."""
    m = fresh_model(make_args(tmp_path, ema_decay=0.5))
    m.change_scale(0)
    m.change_scale(0)
    m.G.alpha = m.D.alpha = 0.5
    assert m.fpD.ema is None
    assert [(k, v.shape) for k, v in m.G_ema.state_dict().items()] == \
        [(k, v.shape) for k, v in m.G.state_dict().items()]
    assert not m.G_ema.training and not any(p.requires_grad for p in m.G_ema.parameters())
    assert torch.equal(m.fpG.ema, m.fpG.flat), "starts as a copy of G"
    live, dead = live_dead(m.fpG)
    assert dead == ["toRGB_blocks.0.toRGB.module.bias", "toRGB_blocks.0.toRGB.module.weight"]
    for step in range(3):
        prev = {n: v.clone() for n, v in m.fpG.eviews.items()}
        m.train_step()
        for n in live:
            assert_one_step(m.fpG.eviews[n], prev[n], m.fpG.views[n], 0.5, (step, n))
        for n in dead:
            assert torch.equal(m.fpG.eviews[n], prev[n]), (step, n)
        assert m.G_ema.alpha == m.G.alpha
    assert not torch.equal(m.fpG.ema, m.fpG.flat)
    sd = m.G_ema.state_dict()
    for n in m.fpG.names:
        assert sd[n].data_ptr() == m.fpG.eviews[n].data_ptr() and torch.equal(sd[n], m.fpG.eviews[n])


def test_average_survives_change_scale_by_name(tmp_path):
    m = fresh_model(make_args(tmp_path, ema_decay=0.5))
    m.change_scale(0)
    for _ in range(2):
        m.train_step()
    old = {n: v.clone() for n, v in m.fpG.eviews.items()}
    assert any(not torch.equal(old[n], m.fpG.views[n]) for n in old)
    m.change_scale(2)
    assert set(m.fpG.eviews) == set(dict(m.G.named_parameters())) and len(m.G_ema.blocks) == 2
    new = [n for n in m.fpG.names if n not in old]
    assert len(new) == 6, new          # the added block's two convs and its toRGB
    for n in old:
        assert torch.equal(m.fpG.eviews[n], old[n]), n
    for n in new:
        assert torch.equal(m.fpG.eviews[n], m.fpG.views[n]), n
    before = {n: m.fpG.eviews[n].clone() for n in new}
    m.G.alpha = m.D.alpha = 0.5        # at alpha 0 the new block gets no gradient yet
    m.train_step()
    for n in new:
        assert not torch.equal(m.fpG.eviews[n], before[n]), n
        assert_one_step(m.fpG.eviews[n], before[n], m.fpG.views[n], 0.5, n)


def _resume(tmp_path, **over):
    args = make_args(tmp_path, ckpt_id="t", **SCHED, **over)
    m = ProgressiveGAN(args, "cpu")
    m.initialize_models()
    m.set_optimizers()
    m.set_dataset()
    m.set_data_iterator()
    m.set_loss_collector()
    m.load_checkpoint()
    return m


def test_checkpoint_round_trip(tmp_path):
    m = fresh_model(make_args(tmp_path, ema_decay=0.5, **SCHED))
    for step in range(4):
        m.check_jump(step)
        m.train_step()
    m.save_checkpoint(3)
    ck = os.path.join(str(tmp_path), "t", "ckpt")
    assert sorted(os.listdir(ck)) == ["D_3.pt", "D_latest.pt", "G_3.pt", "G_ema_3.pt",
                                      "G_ema_latest.pt", "G_latest.pt"]
    sd = torch.load(os.path.join(ck, "G_ema_latest.pt"), weights_only=True)
    g = torch.load(os.path.join(ck, "G_latest.pt"), weights_only=True)
    assert set(sd) == (set(g) - {"optimizer"}) | {"ema_decay"} and sd["ema_decay"] == 0.5
    assert [(k, v.shape) for k, v in sd["model"].items()] == \
        [(k, v.shape) for k, v in m.G.state_dict().items()]
    for k, v in m.G_ema.state_dict().items():
        assert torch.equal(sd["model"][k], v), k
    assert any(not torch.equal(sd["model"][k], g["model"][k]) for k in g["model"])

    m2 = _resume(tmp_path, ema_decay=0.5)
    assert m2.scale_index == m.scale_index == 1 and m2.G_ema.alpha == m.G.alpha
    assert torch.equal(m2.fpG.flat, m.fpG.flat) and torch.equal(m2.fpG.ema, m.fpG.ema)
    # the average goes on from the restored one
    m2._rng_step = m._rng_step
    m.train_step()
    m2.train_step()
    assert torch.equal(m2.fpG.ema, m.fpG.ema)

    # a checkpoint without the file (what the reference writes): the average starts from G
    os.remove(os.path.join(ck, "G_ema_latest.pt"))
    m3 = _resume(tmp_path, ema_decay=0.5)
    assert torch.equal(m3.fpG.ema, m3.fpG.flat)
    for k, v in m3.G.state_dict().items():
        assert torch.equal(m3.G_ema.state_dict()[k], g["model"][k]), k
    # the feature off reads the same checkpoint as before
    m4 = _resume(tmp_path)
    assert m4.G_ema is None and m4.fpG.ema is None


def _tensors(x, path=""):
    if torch.is_tensor(x):
        yield path, x
    elif isinstance(x, dict):
        for k in x:
            if k != "args":
                yield from _tensors(x[k], f"{path}/{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _tensors(v, f"{path}/{i}")


def test_reference_files_do_not_change(tmp_path):
    """G_*.pt and D_*.pt of the same seeded run with the average on and off: the same entries,
    equal tensor for tensor (training is not perturbed, no draw from the global RNG is added),
    and no G_ema file with it off."""
    files = {}
    for name, decay in (("off", None), ("on", 0.999)):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, run_id=name, ema_decay=decay, **SCHED))
        for step in range(4):
            m.check_jump(step)
            m.train_step()
        m.save_checkpoint(3)
        ck = os.path.join(str(tmp_path), name, "ckpt")
        files[name] = sorted(os.listdir(ck))
        files[name + "_sd"] = {n: torch.load(os.path.join(ck, f"{n}_latest.pt"), weights_only=True)
                               for n in "GD"}
    assert files["off"] == ["D_3.pt", "D_latest.pt", "G_3.pt", "G_latest.pt"]
    assert [f for f in files["on"] if "ema" not in f] == files["off"]
    for n in "GD":
        a, b = files["off_sd"][n], files["on_sd"][n]
        assert list(a) == list(b)
        ta, tb = dict(_tensors(a)), dict(_tensors(b))
        assert list(ta) == list(tb) and len(ta) > 10
        for k in ta:
            assert torch.equal(ta[k], tb[k]), (n, k)
        for k in a:
            if k not in ("args", "model", "optimizer"):
                assert a[k] == b[k], (n, k)


# ------------------------------------------------------------------ two ranks, gloo
S, B, ALPHA, DECAY = 1, 4, 0.5, 0.5


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pggan_amd import engine as E
    gsh, dsh = E.g_param_shapes(TINY_DEPTHS, S), E.d_param_shapes(TINY_DEPTHS, S)

    class Pending:   # the overlapped exchange: async all-reduce, mean applied on wait()
        def __init__(self, g):
            self.g, self.w = g, dist.all_reduce(g, async_op=True)

        def wait(self):
            self.w.wait()
            self.g.mul_(1.0 / world)

    def run(flush_each_step):
        PG = {k: torch.from_numpy(v) for k, v in make_params(gsh, seed=501).items()}
        PD = {k: torch.from_numpy(v) for k, v in make_params(dsh, seed=502).items()}
        fpG = E.FlatParams(gsh, E.dead_params("G", S), "cpu", PG, ema=True)
        fpD = E.FlatParams(dsh, E.dead_params("D", S), "cpu", PD)
        eng = E.StepEngine(CpuOps(), TINY_DEPTHS, S, B, "cpu")
        eng.bind(fpG, fpD, E.Hyper(ema_decay=DECAY))
        trail = [(fpG.flat.clone(), fpG.ema.clone())]
        for k in range(3):
            st = make_inputs(B, 4 * 2 ** S, seed=600 + 10 * k + rank)[0]
            eng.train_step(torch.from_numpy(st["real"]), torch.from_numpy(st["z1"]),
                           torch.from_numpy(st["z2"]), ALPHA, ALPHA,
                           grad_hook=lambda net, g: Pending(g))
            if flush_each_step:
                eng.flush()
                trail.append((fpG.flat.clone(), fpG.ema.clone()))
            elif k < 2:
                assert eng._pending_G is not None, "the generator update is deferred"
        eng.flush()
        return trail, fpG

    # the deferred update landing inside the next step (Adam_G + average in _finish_G) ...
    _, fp = run(False)
    # ... and completed by flush() after every step, which exposes each post-step G
    trail, fp2 = run(True)
    torch.save(dict(ema=fp.ema, flat=fp.flat, ema2=fp2.ema, trail=trail),
               os.path.join(out_dir, f"ema{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_overlapped_exchange(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"ema{i}.pt", weights_only=True) for i in range(world)]
    assert torch.equal(r[0]["ema"], r[1]["ema"]) and torch.equal(r[0]["flat"], r[1]["flat"])
    for o in r:
        assert torch.equal(o["ema"], o["ema2"]), "deferred into the next step == flushed"
        trail = o["trail"]
        assert len(trail) == 4 and torch.equal(trail[0][0], trail[0][1])
        assert torch.equal(trail[3][0], o["flat"])
        for k in range(1, 4):
            assert not torch.equal(trail[k][1], trail[k - 1][1])
            assert_one_step(trail[k][1], trail[k - 1][1], trail[k][0], DECAY, k)
