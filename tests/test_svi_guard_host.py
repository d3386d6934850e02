"""What a captured SVI step freezes on the host, and the guards around it: pre-arming is
opt-in, the Python scalars a model / guide can reach are watched, the parameter store has a generation.
The reference re-runs the model on every step (pyro/infer/svi.py:134-162), so it needs none of this; a
backend that replays a graph has to notice what the reference would have seen."""
import functools

import torch

import pyro_amd as pyro
from pyro_amd.infer import SVI, Trace_ELBO
from pyro_amd.infer import svi as svi_mod


def test_prearm_is_opt_in():
    class _Optim:
        zeroes_grads = True

        def __call__(self, params, *a, **k):
            pass
    for kw, want in (({}, False), ({"hip_graph": True}, False), ({"prearm": True, "hip_graph": True}, True)):
        s = SVI(lambda: None, lambda: None, _Optim(), Trace_ELBO(), **kw)
        assert s.prearm is want, kw


def test_a_replay_given_up_is_noticed_when_its_stand_in_has_already_published():
    """The released replay gave itself up (ack == its number) and the replay armed behind it ran as this
    step and published BEFORE read_loss looked once: nothing waits behind the gate any more, so the entry
    may not go on believing that a replay is armed (the step after would release a replay that is not
    there).  Without a give-up the same call leaves the armed replay armed."""
    import types

    import numpy as np

    def entry_after(ack):
        mailbox = (torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
        e = svi_mod._CapturedStep(None, None, None, mailbox=mailbox)
        e.gate = types.SimpleNamespace(go_np=np.full(1, 2), ack_np=np.full(1, ack), next=2)
        e.armed = True                      # (the replay enqueued for the step after this one)
        mailbox[0][0], mailbox[1][0] = 1.5, 7          # ... has published as this step
        assert e.read_loss(released_armed=True) == 1.5 and e.gate.next == 3
        return e

    e = entry_after(ack=2)
    assert not e.armed and e.arm_backoff == 1 and e.arm_penalty == 2
    e = entry_after(ack=1)                  # (an earlier give-up, long dealt with)
    assert e.armed and e.arm_backoff == 0 and e.arm_penalty == 1


BETA = 0.5


def test_watch_sees_closures_globals_partials_attributes_and_module_flags():
    scale = 2.0

    def closure_model(x):
        return x * scale * BETA

    class Obj:
        def __init__(self):
            self.beta, self.name, self.t = 1.0, "a", torch.zeros(1)

        def __call__(self, x):
            return x * self.beta

    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Dropout(0.5))

    class WithNet:
        def __init__(self):
            self.net = net

        def model(self, x):
            return self.net(x)

    o, w = Obj(), WithNet()
    part = functools.partial(closure_model)
    watch = svi_mod._host_scalar_watch(part, o, w.model, net)
    names = {k for _, k, _ in watch[0]}
    assert {"BETA", "beta", "name", "training"} <= names and len(watch[1]) == 1
    assert svi_mod._host_scalars_changed(watch) is None
    o.beta = 0.25
    assert svi_mod._host_scalars_changed(watch) == "beta"
    o.beta = 1.0
    assert svi_mod._host_scalars_changed(watch) is None
    net.eval()
    assert svi_mod._host_scalars_changed(watch) == "training"
    net.train()
    global BETA
    BETA = 0.75
    assert svi_mod._host_scalars_changed(watch) == "BETA"
    BETA = 0.5
    scale = 3.0                          # noqa: F841  (the closure cell of closure_model)
    assert svi_mod._host_scalars_changed(watch) == "<closure>"


def test_watch_of_the_bench_model_is_small():
    from pyro_amd import examples
    from pyro_amd.infer.autoguide import AutoNormal
    guide = AutoNormal(examples.logreg_model, init_scale=0.1)
    maps, cells = svi_mod._host_scalar_watch(examples.logreg_model, guide)
    assert len(maps) + len(cells) < 64          # (compared before every replay)


def test_param_store_generation_moves_with_the_set_of_leaves():
    pyro.clear_param_store()
    store = pyro.get_param_store()
    g0 = store.generation
    pyro.param("a", torch.zeros(2))
    g1 = store.generation
    assert g1 > g0
    pyro.param("a")                       # a read creates nothing
    pyro.param("a", torch.ones(2))        # nor does an init for an existing name
    assert store.generation == g1
    with store.scope():
        assert store.generation > g1
    g2 = store.generation
    del store["a"]
    assert store.generation > g2
    g3 = store.generation
    pyro.clear_param_store()
    assert store.generation > g3


def test_torch_rng_state_restores_rewind_the_philox_stream():
    """the kernels' Philox position follows the default generator not only through
    torch.manual_seed but through torch.get_rng_state / set_rng_state and torch.random.fork_rng as well --
    restoring the generator replays the draws, as it does in the reference (pyro/util.py:48-63)."""
    from pyro_amd import rng
    pyro.set_rng_seed(5)
    rng.reserve(1000, torch.float32)
    at = rng._STATE["offset"]
    state = torch.get_rng_state()
    rng.reserve(4000, torch.float32)
    assert rng._STATE["offset"] == at + 1000
    torch.set_rng_state(state)                              # the same tensor object: matched by identity
    assert rng._STATE["offset"] == at and rng.current_seed() == 5
    with torch.random.fork_rng(devices=[]):
        rng.reserve(999, torch.float32)
        torch.rand(3)
    assert rng._STATE["offset"] == at
    copy = torch.get_rng_state().clone()                    # a copy: matched by its bytes
    rng.reserve(8, torch.float32)
    torch.set_rng_state(copy)
    assert rng._STATE["offset"] == at
    # a state this process never handed out re-seeds the generator: the stream restarts under its seed
    torch.set_rng_state(torch.Generator().manual_seed(99).get_state())
    assert rng.current_seed() == 99 and rng._STATE["offset"] == 0
    # pyro's own pair carries the position explicitly
    pyro.set_rng_seed(7)
    rng.reserve(64, torch.float32)
    full = pyro.util.get_rng_state()
    rng.reserve(64, torch.float32)
    pyro.util.set_rng_state(full)
    assert rng._STATE["offset"] == 16 and rng.current_seed() == 7
