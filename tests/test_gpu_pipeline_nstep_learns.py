"""The learning test of the batched learner on n-step returns ("n-step returns"): the configuration of
tests/test_gpu_pipeline_learns.py with n_step = 10 still beats the zero action on the held-out fields."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, EPISODES, B, N_STEP = 51, 60, 64, 10


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ten_step_returns_beat_the_zero_action(pkg, seed):
    """KS22 geometry, B = 64, fp32, 51-step episodes from a new random field each (random_init), exploration noise 0.3, graphs
    on, 60 episodes, the diagonal target (quirk_target_broadcast=False) in the setup's default target regime (frozen), n_step = 10;
    a greedy evaluation on 64 held-out fields every 10 episodes, the best actor chosen by it.  Asserted: the best evaluation score
    is above the zero action's on the same fields.

    n_step = 10 is the one n > 1 of tools/nstep_probe.py's table for which all three seeds do so under frozen targets (n = 3 and
    n = 5 fail in seed 2); n = 10 scores below n = 1 in every seed of that table (-0.737 / -1.351 / -0.787), so this pins that
    the n-step learner learns, not that it learns better.

    Measured once: best score -3.880 (episode 60) / -4.300 (60) / -4.128 (50) for seeds 0 / 1 / 2, against -6.889
    for the zero action."""
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(seed), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7 + seed, trajectory_length=1, quirk_target_broadcast=False)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    p = pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                          noise_seed=99 + seed, log_episodes=EPISODES, random_init=True, init_seed=1 + seed, eval_every=10,
                          eval_inits=64, eval_seed=10_000, best_by="eval", n_step=N_STEP)
    assert p.use_graphs and p.n_step == N_STEP
    p.run(5)
    p.capture()
    p.run(EPISODES * E - p.tick)
    p.sync()
    eps, _, blew, _ = p.eval_returns()
    scores = p.eval_scores
    print(f"seed {seed}: zero action {p.eval_zero_score:.4f}, evaluations {dict(zip(eps.tolist(), np.round(scores, 4).tolist()))}, "
          f"best {p.bestreward:.4f} at episode {p.bestepisode}, graph launches {p.n_graph_launches}")
    assert p.n_episodes == EPISODES and eps.tolist() == [10, 20, 30, 40, 50, 60] and p.n_graph_launches > 0
    assert np.isfinite(p.eval_zero_score)
    assert p.bestepisode > 0 and p.bestreward > p.eval_zero_score
    p.close()
