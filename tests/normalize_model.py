"""NumPy float64 model of the engine's normalization (sg_set_normalize): gym 0.21's NormalizeObservation / NormalizeReward for
a vector env (gym/wrappers/normalize.py), with the engine's documented choices -- statistics and normalized values in
float64, each output rounded to float32 once, terminal observations normalized with the statistics of their own step."""
import numpy as np


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.update_from_moments(np.mean(x, axis=0), np.var(x, axis=0), x.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        M2 = m_a + m_b + np.square(delta) * self.count * batch_count / tot_count
        self.var = M2 / tot_count
        self.mean = new_mean
        self.count = tot_count


def _clip(v, c):
    return v if c is None else np.clip(v, -c, c)


class NormalizeModel:
    """feed it the raw outputs of a twin handle (same seed and actions, normalization off); it returns what the handle with
    normalization on must return"""

    def __init__(self, num_envs, obs_dim, obs=True, reward=True, gamma=0.99, epsilon=1e-8, clip_obs=None, clip_reward=None,
                 update=True):
        self.obs_rms, self.ret_rms = RunningMeanStd((obs_dim,)), RunningMeanStd(())
        self.returns = np.zeros(num_envs, np.float64)
        self.obs, self.reward, self.gamma, self.epsilon = obs, reward, gamma, epsilon
        self.clip_obs, self.clip_reward, self.update = clip_obs, clip_reward, update

    def norm_obs(self, o):
        o = np.asarray(o, np.float64)
        return _clip((o - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), self.clip_obs).astype(np.float32)

    def reset(self, obs):
        if not self.obs:
            return np.asarray(obs, np.float32)
        if self.update:
            self.obs_rms.update(obs)
        return self.norm_obs(obs)

    def step(self, obs, reward, done, terminal_obs=None):
        """one step row: (obs, reward, normalized terminal rows or None); terminal_obs: rows to normalize with this step's
        statistics (they do not enter the update)"""
        out_obs, out_rew, out_t = np.asarray(obs, np.float32), np.asarray(reward, np.float32), terminal_obs
        if self.obs:
            if self.update:
                self.obs_rms.update(obs)
            out_obs = self.norm_obs(obs)
            if terminal_obs is not None:
                out_t = self.norm_obs(terminal_obs)
        if self.reward:
            if self.update:
                self.returns = self.returns * self.gamma + np.asarray(reward, np.float64)
                self.ret_rms.update(self.returns)
            out_rew = _clip(np.asarray(reward, np.float64) / np.sqrt(self.ret_rms.var + self.epsilon), self.clip_reward).astype(np.float32)
            if self.update:
                self.returns[np.asarray(done, bool)] = 0.0
        return out_obs, out_rew, out_t
