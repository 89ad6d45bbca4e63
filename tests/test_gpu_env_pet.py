"""`env.encroachment_log()` (copo_amd/torch_copo/utils/env_wrappers.py): created on first use, recording after reset and step next to the
other observers, replaced by a call with arguments, closed by `close()`, and equal to a stand-alone log fed the same states."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_env_encroachment_log_attaches_late_and_matches_a_log_by_hand():
    import torch
    from copo_amd import observers as ob
    from copo_amd.encroach import EncroachmentLog
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    assert "encroachment_log" not in MultiAgentIntersectionEnv.default_config() and all(r.key != "encroachment_log" for r in ob.ENV_OBSERVERS)
    env = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2, trip_log={}))
    other = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2))
    log = None
    try:
        act = torch.zeros(2, env.sim.N, 2, device="cuda")
        act[..., 1] = torch.linspace(0.3, 1.0, env.sim.N, device="cuda")
        env.vec_reset()
        other.vec_reset()
        for _ in range(5):
            env.vec_step(act)
            other.vec_step(act)
        assert env.observer("encroachment_log") is None
        mine = env.encroachment_log(window=30, max_rows=4096)
        log = EncroachmentLog.for_map(other.sim, window=30, max_rows=4096)
        log.record()
        at = env.observers.records
        assert mine.n_records == 1 and env.encroachment_log() is mine and env.observers.names() == ["trip_log", "encroachment_log"]
        assert (mine.W, mine.H, mine.x0, mine.y0) == (log.W, log.H, log.x0, log.y0)
        for k in range(2):
            for _ in range(40):
                env.vec_step(act)
                other.vec_step(act)
                log.record()
            assert mine.n_records == 1 + env.observers.records - at
            if k == 0:
                env.vec_reset()
                other.vec_reset()
                log.forget()                             # what `env_record` does after a reset
                log.record()
        assert mine.n_records == log.n_records == 82
        a, b = mine.table(), log.table()
        assert len(a) > 0 and a.meta["dropped"] == 0 and np.array_equal(a.raw, b.raw)
        ga, gb = mine.aggregates(), log.aggregates()
        assert np.array_equal(ga["hist"], gb["hist"]) and np.array_equal(ga["critical"], gb["critical"]) and ga["hist"].sum() == len(a)
        assert all(np.array_equal(x, y) for x, y in zip(mine.memory(), log.memory()))
        # the join with the trip log of the same env
        env.trip_log().flush()
        j = a.join(env.trip_log().table())
        assert (j["second"] >= 0).any() and j["missing"] < 2 * len(a)
        # arguments make a new log, which replaces (and closes) the first
        new = env.encroachment_log(max_rows=16)
        assert new is not mine and not mine._h.value and env.encroachment_log() is new and new.n_records == 1
    finally:
        if log is not None:
            log.close()
        other.close()
        env.close()
    assert env.observer("encroachment_log") is None and not new._h.value
