"""CPU: the streaming validation rollout (lns_rollout_eval & co., include/lns.h) is declared and exported, refuses bad
arguments before any device work, and `parallel.ShardedEval` gathers only the reductions (gloo, world size 2)."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT

EVAL_SYMBOLS = ("lns_rollout_eval", "lns_rollout_latent_eval", "lns_rollout_eval_workspace_bytes")


def test_eval_symbols_are_declared_and_exported():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in EVAL_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
    assert "lns_eval_spec" in src and re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)


def _engine():
    from lns_amd import config, engine
    return engine.Engine(engine.make_config(config.preset("ns2d_mini"), ae_prefix="vq_ae.", prop_prefix="propagator."))


def test_eval_entry_points_refuse_bad_arguments_without_a_device():
    """Every LNS_EINVAL case is decided before the first HIP call: this runs on a machine without a GPU, with fake
    (never dereferenced) device pointers."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    e = _engine()
    h = e._h
    spec = engine.eval_spec(2, mean=0.37, std=1.9)
    sp = ctypes.byref(spec)
    P = ctypes.c_void_p(0x1000)                       # stands for a device pointer
    keep = (ctypes.c_int * 3)(0, 3, 4)
    n = ctypes.c_size_t(0)

    def err():
        return L.lns_last_error(h).decode()

    def ev(eng=h, x=P, y=P, B=3, T=5, s=sp, frame=P, seq=P, k=keep, nk=3, frames=P):
        return L.lns_rollout_eval(eng, x, None, y, B, T, s, frame, seq, k, nk, frames, P, 1 << 30, None)

    def lev(eng=h, z=P, y=P, B=3, T=2, t0=0, Ttot=5, s=sp, frame=P, seq=P, k=None, nk=0, frames=None):
        return L.lns_rollout_latent_eval(eng, z, None, y, B, T, t0, Ttot, s, frame, seq, k, nk, frames, None, P, 1 << 30, None)

    assert ev(eng=None) == _lib.LNS_EINVAL and lev(eng=None) == _lib.LNS_EINVAL
    assert L.lns_rollout_eval_workspace_bytes(None, 3, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_rollout_eval_workspace_bytes(h, 0, ctypes.byref(n)) == _lib.LNS_EINVAL and "B" in err()
    for kw, word in ((dict(x=None), "x"), (dict(y=None), "y_true"), (dict(B=0), "B"), (dict(B=-2), "B"), (dict(T=0), "T"),
                     (dict(frame=None, seq=None), "frame_out"), (dict(s=None), "spec"),
                     (dict(k=(ctypes.c_int * 3)(0, 4, 3)), "keep_steps"), (dict(k=(ctypes.c_int * 3)(0, 3, 3)), "keep_steps"),
                     (dict(k=(ctypes.c_int * 3)(0, 3, 5)), "keep_steps"), (dict(k=(ctypes.c_int * 3)(-1, 3, 4)), "keep_steps"),
                     (dict(k=None), "keep_steps"), (dict(frames=None), "frames_out"), (dict(nk=-1), "n_keep")):
        assert ev(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    for kw, word in ((dict(z=None), "z_in"), (dict(y=None), "y_true"), (dict(B=0), "B"), (dict(T=0), "T"),
                     (dict(frame=None, seq=None), "frame_out"), (dict(t0=-1), "t0"), (dict(t0=4), "t0"),
                     (dict(Ttot=1), "T_total"), (dict(k=(ctypes.c_int * 2)(1, 0), nk=2, frames=P), "keep_steps"),
                     (dict(k=(ctypes.c_int * 1)(2), nk=1, frames=P), "keep_steps")):
        assert lev(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    bad = engine.eval_spec(2)
    bad.size = 8                                      # a struct of another version
    assert ev(s=ctypes.byref(bad)) == _lib.LNS_EINVAL and "spec" in err()
    # the horizon is bounded by the "eval_max_steps" option (it sizes the partial sums of the workspace)
    e.set_option("eval_max_steps", 4)
    assert ev() == _lib.LNS_EINVAL and "eval_max_steps" in err()
    with pytest.raises(_lib.LnsError):
        e.set_option("eval_max_steps", 0)


def test_eval_spec_follows_the_rule_of_relative_l2():
    from lns_amd import engine, metrics
    s = engine.eval_spec(3, mean=0.37, std=1.9)
    assert s.per_channel == 0 and s.size == ctypes.sizeof(s) and abs(s.mean - 0.37) < 1e-7
    s = engine.eval_spec(3, mean=[0.4, -0.2, 9.5], std=[2.1, 1.7, 0.6])
    assert s.per_channel == 1 and list(s.flags_c) == [0] * 8 and abs(s.std_c[2] - 0.6) < 1e-7 and s.std_c[5] == 1.0
    s = engine.eval_spec(4, **metrics.twophase_spec(0.013, 0.21, 310.0, 180.0))
    assert s.per_channel == 1 and list(s.flags_c)[:4] == [1, 1, 0, 2] and s.clamp_lo == 0.0
    with pytest.raises(ValueError):
        engine.eval_spec(3, mean=[0.0, 1.0])


def test_validate_refuses_cpu_tensors():
    from lns_amd import config, dropin
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    with pytest.raises(Exception) as ei:
        m.validate(torch.zeros(2, 2, 32, 32), torch.zeros(2, 3, 2, 32, 32), mean=0.1, std=2.0)
    assert "no CPU fallback" in str(ei.value)


def test_build_staleness_covers_inc_files(monkeypatch):
    """_lib.build() rebuilds when an included kernel source (*.inc) is newer than the library."""
    from lns_amd import _lib
    _lib.build()
    calls = []
    monkeypatch.setattr(_lib.subprocess, "check_call", lambda *a, **k: calls.append(a))
    _lib.build()
    assert not calls                                   # up to date
    lib_mtime = os.path.getmtime(_lib.LIB_PATH)
    real = os.path.getmtime

    def newer_inc(p):
        return lib_mtime + 10 if p.endswith("fa_fused.inc") else real(p)
    monkeypatch.setattr(_lib.os.path, "getmtime", newer_inc)
    _lib.build()
    assert len(calls) == 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_eval_worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lns_oracle
    from helpers import METRIC_STATS, metric_inputs
    from lns_amd import parallel
    st = METRIC_STATS["ns2d"]
    yh, y = metric_inputs("ns2d")                               # global batch of 2: one trajectory per rank

    def evaluate(yh_shard, y_shard):                            # per-rank reduction: the oracle on CPU, fp32 like the engine's
        f, s = lns_oracle.rollout_metrics(yh_shard.numpy(), y_shard.numpy(), st["mean"], st["std"])
        return torch.from_numpy(f.astype(np.float32)), torch.from_numpy(s.astype(np.float32))

    se = parallel.ShardedEval(evaluate, yh.shape[0])
    f_all, s_all = se.run(torch.from_numpy(yh), torch.from_numpy(y))
    if rank == 0:
        f_ref, s_ref = lns_oracle.rollout_metrics(yh, y, st["mean"], st["std"])
        q.put((tuple(f_all.shape), tuple(s_all.shape), bool((f_all.numpy() == f_ref.astype(np.float32)).all()),
               bool((s_all.numpy() == s_ref.astype(np.float32)).all()), se.bytes_received_per_rank,
               se.bytes_contributed_per_rank, (se.lo, se.hi)))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_eval_gathers_only_the_reductions():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_eval_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    fshape, sshape, f_ok, s_ok, received, contributed, span = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    B, T, C = 1, 5, 3                                           # per rank
    assert fshape == (2, T, C) and sshape == (2, C) and span == (0, 1)
    assert f_ok and s_ok                                        # per-trajectory reductions: sharded == unsharded, exactly
    assert received == 4 * (B * T * C + B * C) * (2 - 1)        # the other rank's reductions, nothing else
    assert contributed == 4 * (B * T * C + B * C)
