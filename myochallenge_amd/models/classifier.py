"""Task classifier of the winning ensemble (/root/reference/src/models/classifier.py), its data collection and its training.

A 234 -> 200 -> 100 -> 1 ReLU MLP on the first N_OBS_PER_TRIAL = 13 observations' slice [29:47]
(object-2 position / velocity, both targets and their errors: DIMS_PER_OBS = 18), standardised with a
scikit-learn ``StandardScaler``; ``round(sigmoid(logit)) == 0`` means the HOLD task
(src/eval_mixture_of_ensembles.py:186-188).  Layer names match the reference so ``classifier.pt`` loads
unchanged; the scaler pickle is read and written without scikit-learn.

Collection (``DataCollector``, classifier.py:67-121) runs the reference's trials as ONE batch: N envs = N trials,
each reset and then stepped 50 times through the UNWRAPPED step (``myo_batch_step_inner``: no TimeLimit, no
auto-reset; an env that drops a ball keeps stepping, only the policy's LSTM state restarts, as in the
reference's loop over a bare gym env).  The whole collection stays on the device.  Trial t runs in env slot
t mod N at that slot's (t div N)-th reset, so its reset draws and physics are those of the Philox stream
(seed, t mod N, episode); the exploration noise comes from a generator seeded with ``seed``.  One difference from the
reference's single env: there a HOLD trial inherits the target sites where the previous trial left them (a reset does
not move them and a HOLD goal never turns); here every trial starts with the targets of a freshly made env, so that
no trial depends on another and each can be replayed alone.

Training (``train_task_classifier``, classifier.py:187-269) restates scikit-learn's ``train_test_split`` and
``StandardScaler`` in numpy and runs the reference's loop (BCEWithLogitsLoss, Adam, 40 epochs of batch 100
drawn by ``DataLoader(shuffle=True)``) with torch on the chosen device.
"""
from __future__ import annotations

import math
import os
import pickle
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

N_OBS_PER_TRIAL = 13
DIMS_PER_OBS = 18
OBS_SLICE = (29, 47)          # src/eval_mixture_of_ensembles.py:181
ENV_NAME = "CustomMyoBaodingBallsP2"
LEARNING_RATE = 0.01
N_EPOCHS = 40
BATCH_SIZE = 100
TEST_SIZE, SPLIT_SEED = 0.10, 69                 # train_test_split(X, y, test_size=0.10, random_state=69)
SKLEARN_VERSION = "1.1.2"                        # what tests/golden/classifier_scaler.pkl was written by


class TaskClassifier(torch.nn.Module):
    def __init__(self, n_obs_per_trial: int = N_OBS_PER_TRIAL):
        super().__init__()
        self.layer_1 = torch.nn.Linear(n_obs_per_trial * DIMS_PER_OBS, 200)
        self.layer_2 = torch.nn.Linear(200, 100)
        self.layer_out = torch.nn.Linear(100, 1)
        self.activation = torch.nn.ReLU()

    def forward(self, x):
        x = self.activation(self.layer_1(x))
        x = self.activation(self.layer_2(x))
        return self.layer_out(x)

    @torch.no_grad()
    def predict_task(self, x) -> torch.Tensor:
        """0 = HOLD, 1 = rotating task (update_task, src/eval_mixture_of_ensembles.py:186-188)."""
        return torch.round(torch.sigmoid(self(x))).reshape(-1).to(torch.long)


class _Stub:
    def __setstate__(self, s):
        self.__dict__.update(s if isinstance(s, dict) else {"_state": s})


class _ScalerUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.split(".")[0] in ("numpy", "builtins", "collections", "copyreg", "_codecs"):
            return super().find_class(module, name)
        return type(name, (_Stub,), {"__module__": module})


def load_scaler(path: str):
    """(mean, scale) float64 arrays of a pickled sklearn StandardScaler: transform(x) = (x - mean) / scale."""
    with open(path, "rb") as fh:
        sc = _ScalerUnpickler(fh).load()
    mean = np.asarray(sc.mean_, np.float64) if getattr(sc, "with_mean", True) else np.zeros_like(sc.scale_)
    scale = np.asarray(sc.scale_, np.float64) if getattr(sc, "with_std", True) else np.ones_like(mean)
    return mean, scale


# ---------------------------------------------------------------------------------------------------- data collection


def get_config() -> dict:
    """The env config of the collection (classifier.py:29-43): only `solved` is rewarded, the task is drawn per episode."""
    return {
        "weighted_reward_keys": {"pos_dist_1": 0, "pos_dist_2": 0, "act_reg": 0, "alive": 0, "solved": 5, "done": 0, "sparse": 0},
        "goal_time_period": (4, 6),
        "task_choice": "random",
        "goal_xrange": (0.020, 0.030),
        "goal_yrange": (0.022, 0.032),
    }


def load_model_and_env(model_path: str, env_path: str, env):
    """(policy, VecNormalize over ``env``) of a recurrent SB3 zip and its VecNormalize pickle (classifier.py:46-63).  The
    reference's custom_objects (learning rate and clip range 0) only disarm training; the policy here is inference-only."""
    from ..rl.sb3_zip import load_policy
    from ..rl.vec_normalize import VecNormalize
    policy = load_policy(model_path)[0]
    if not policy.recurrent:
        raise ValueError(f"{model_path}: the collection policy must be recurrent (MlpLstmPolicy)")
    norm = VecNormalize.load(env_path, env)
    norm.training = False
    norm.norm_reward = False
    return policy.to(env.device).eval(), norm


@dataclass
class DataCollector:
    """Collects classifier trials with a recurrent policy (classifier.py:67-121), batched: ``collect_data(env, n)`` runs
    n trials in chunks of ``env.num_envs``.  The raw windows land in one preallocated [n, 50, 18] device tensor."""
    model_path: str
    env_path: str
    seed: int = 0                 # seed of the exploration noise generator
    timestep = 0
    n_obs_per_trial = 50

    def __post_init__(self):
        self.model, self.env = None, None          # bound to an env by collect_data (VecNormalize needs its device / obs size)
        self._bound = None
        self.all_obs, self.task_ids = [], []

    def _bind(self, env) -> None:
        if self._bound is not env:
            self.model, self.env = load_model_and_env(self.model_path, self.env_path, env)
            self._bound = env

    @staticmethod
    def _fresh_targets(env) -> torch.Tensor:
        """target1 / target2 xy (palm frame) of a newly created env of ``env``'s model and task: task_d[5:9] of a one-env batch."""
        from .. import native
        one = native.Batch(env._model, env._cfg, 1, env.device.index or 0, 0, env.dtype)
        try:
            td = torch.zeros((1, 9), dtype=torch.float64, device=env.device)
            one.get_task(None, td, None, env._stream())
        finally:
            one.close()
        return td[0, 5:9].clone()

    def predict(self, obs, state, episode_start, deterministic):
        """model.predict(env.normalize_obs(obs), ...) on device tensors: the clipped action and the new LSTM state."""
        self.timestep += 1
        a, _, _, state = self.model.act(self.env.normalize_obs(obs), state, episode_start, deterministic=deterministic)
        return torch.clamp(a, -1.0, 1.0).to(torch.float32).contiguous(), state

    @torch.no_grad()
    def collect_data(self, env, n_episodes: int = 10_000, *, deterministic: bool = False, return_actions: bool = False):
        """n_episodes trials of n_obs_per_trial steps.  Returns (windows float32 [n, 50, 18], task ids int64 [n], actions float32
        [n, 50, nu] or None), device tensors; no host synchronisation inside the loop."""
        self._bind(env)
        dev, N, T = env.device, env.num_envs, self.n_obs_per_trial
        lo_s, hi_s = OBS_SLICE
        n = int(n_episodes)
        windows = torch.empty((n, T, hi_s - lo_s), dtype=torch.float32, device=dev)
        tasks = torch.empty(n, dtype=torch.int64, device=dev)
        acts = torch.empty((n, T, env.act_dim), dtype=torch.float32, device=dev) if return_actions else None
        done = torch.zeros(N, dtype=torch.uint8, device=dev)
        task_i = torch.zeros((N, 2), dtype=torch.int32, device=dev)
        task_d = torch.zeros((N, 9), dtype=torch.float64, device=dev)
        ball_d = torch.zeros((N, 10), dtype=torch.float64, device=dev)
        fresh_targets = self._fresh_targets(env)
        gen = torch.Generator(device=dev).manual_seed(int(self.seed))
        pol = self.model                                  # (the collector's own copy: its exploration noise comes from gen)
        pol.noise_fn = lambda mean: torch.randn(mean.shape, generator=gen, device=mean.device, dtype=mean.dtype)
        for lo in range(0, n, N):
            k = min(N, n - lo)
            # a HOLD episode never moves the target sites (the goal only turns while rotating), so a reset keeps where the
            # slot's last trial left them; put them back where a freshly made env has them, so that no trial depends on another
            env.batch.get_task(task_i, task_d, ball_d, env._stream())
            task_d[:, 5:9] = fresh_targets
            env.batch.set_task(task_i, task_d, ball_d, env._stream())
            obs = env.reset_tensor()                  # env slot i: its next episode of the (seed, i, episode) stream
            if pol.use_sde:
                pol.reset_noise(N, generator=gen)
            state = pol.initial_state(N, dev)
            starts = torch.ones(N, dtype=torch.float32, device=dev)
            for t in range(T):
                windows[lo:lo + k, t] = obs[:k, lo_s:hi_s]          # the raw observation before the step
                a, state = self.predict(obs, state, starts, deterministic)
                if acts is not None:
                    acts[lo:lo + k, t] = a[:k]
                env.batch.step_inner(None, a, obs, done, env._stream())      # the unwrapped env.step: no reset inside a trial
                starts = done.to(torch.float32)                               # episode_starts = dones
            env.batch.get_task(task_i, None, None, env._stream())
            tasks[lo:lo + k] = task_i[:k, 0].to(torch.int64)                 # env.which_task at the end of the trial
        self.all_obs.append(windows)
        self.task_ids.append(tasks)
        return windows, tasks, acts

    def save_data(self, path) -> None:
        """The reference's CSV (``pd.DataFrame(np.vstack(all_obs)); df["task_id"] = task_ids; df.to_csv(path, index=False)``)."""
        X = torch.cat([w.reshape(w.shape[0], -1) for w in self.all_obs]).cpu().numpy()
        y = torch.cat(self.task_ids).cpu().numpy()
        write_csv(path, X, y)


def write_csv(path, X: np.ndarray, task_ids: np.ndarray) -> None:
    """Header ``0,1,...,{d-1},task_id`` then one row per trial; floats with 9 significant digits (float32 round trip)."""
    X = np.asarray(X, np.float32)
    d = X.shape[1]
    data = np.concatenate([X.astype(np.float64), np.asarray(task_ids, np.float64).reshape(-1, 1)], axis=1)
    with open(path, "w", encoding="utf8", newline="\n") as fh:
        fh.write(",".join([str(j) for j in range(d)] + ["task_id"]) + "\n")
        np.savetxt(fh, data, fmt=["%.9g"] * d + ["%d"], delimiter=",")


def read_csv(path, n_columns: Optional[int] = None):
    """(X float64 [n, n_columns or all], task_id int64 [n]) of a CSV written by save_data or by the reference (pandas)."""
    with open(path, encoding="utf8") as fh:
        header = fh.readline().strip().split(",")
    if header[-1] != "task_id":
        raise ValueError(f"{path}: the last column is {header[-1]!r}, not 'task_id'")
    d = len(header) - 1
    cols = list(range(d if n_columns is None else int(n_columns))) + [d]
    a = np.loadtxt(path, delimiter=",", skiprows=1, usecols=cols, dtype=np.float64, ndmin=2)
    return a[:, :-1], a[:, -1].astype(np.int64)


def collect_data_for_classifier(model_path: str, env_path: str, save_path: str, n_episodes: int = 10_000, *,
                                num_envs: int = 4096, seed: int = 0, device: int = 0) -> DataCollector:
    """classifier.py:124-133: collect n_episodes trials with the policy (model zip + VecNormalize pickle) and write the CSV."""
    from ..envs.environment_factory import EnvironmentFactory
    env = EnvironmentFactory.create(ENV_NAME, num_envs=int(min(num_envs, n_episodes)), seed=seed, device=device, **get_config())
    try:
        print("\n\nCollecting data\n")
        start = time.time()
        data_collector = DataCollector(model_path, env_path, seed=seed)
        data_collector._bind(env)                       # (policy and normaliser loads are not part of the collection's time)
        t0 = time.time()
        data_collector.collect_data(env, n_episodes=n_episodes)
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
        t1 = time.time()
        data_collector.save_data(save_path)
        steps = n_episodes * data_collector.n_obs_per_trial
        print(f"Collected {n_episodes} trials x {data_collector.n_obs_per_trial} steps in {t1 - t0:.3f} s "
              f"({n_episodes / (t1 - t0):.0f} trials/s, {steps / (t1 - t0):.3g} env-steps/s); CSV written in {time.time() - t1:.3f} s")
        print(f"Data collection took {time.time() - start:.3f} s")
    finally:
        env.close()
    return data_collector


# ---------------------------------------------------------------------------------------------------- training


def train_test_split_indices(n: int, test_size: float = TEST_SIZE, random_state: int = SPLIT_SEED):
    """(train, test) row indices of sklearn's ``train_test_split(..., test_size, random_state)`` (ShuffleSplit: the first
    ceil(test_size n) entries of RandomState(random_state).permutation(n) are the test set)."""
    n_test = int(math.ceil(test_size * n))
    perm = np.random.RandomState(random_state).permutation(n)
    return perm[n_test:], perm[:n_test]


def fit_scaler(X: np.ndarray) -> dict:
    """The fitted state of sklearn's ``StandardScaler().fit(X)`` on dense float64 data: mean, population variance and
    scale = sqrt(var), 1 where the feature is constant (sklearn's _is_constant_feature bound)."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    dev_ = X - mean
    var = ((dev_ ** 2).sum(axis=0) - dev_.sum(axis=0) ** 2 / n) / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return {"with_mean": True, "with_std": True, "copy": True,
            "feature_names_in_": np.array([str(j) for j in range(X.shape[1])], dtype=object),
            "n_features_in_": int(X.shape[1]), "n_samples_seen_": np.int64(n),
            "mean_": mean, "var_": var, "scale_": scale, "_sklearn_version": SKLEARN_VERSION}


def save_scaler(path, state: dict) -> None:
    """Pickle a StandardScaler state so that scikit-learn revives it as ``sklearn.preprocessing._data.StandardScaler``."""
    from ..rl.sb3_pickle import instance, stand_ins
    with stand_ins([("sklearn.preprocessing._data", "StandardScaler", "object")]) as cls:
        obj = instance(cls[("sklearn.preprocessing._data", "StandardScaler")], state)
        with open(path, "wb") as fh:
            pickle.dump(obj, fh, protocol=4)


def binary_acc(y_pred, y_test):
    """Batch accuracy in whole percent (classifier.py:177-184)."""
    y_pred_tag = torch.round(torch.sigmoid(y_pred))
    acc = (y_pred_tag == y_test).sum().float() / y_test.shape[0]
    return torch.round(acc * 100)


def train_task_classifier(data_path: str = "../output/classifier/data_for_baoding_task_classifier_alberto-518.csv",
                          save_folder: Optional[str] = None, *, seed: int = 0, device=None, n_epochs: int = N_EPOCHS,
                          verbose: bool = True) -> dict:
    """classifier.py:187-269.  Reads the CSV, keeps the first 13 x 18 columns, y = clip(task_id, 0, 1) (HOLD vs rotate),
    splits 90/10 as train_test_split(random_state=69), standardises, trains TaskClassifier and writes
    ``task_classifier.pt`` and ``scaler.pkl`` into save_folder (default: the CSV's directory).  The weights are
    initialised under torch.manual_seed(seed) and the batches drawn by DataLoader(shuffle=True) with a
    torch.Generator seeded with seed.  Returns the test accuracy, the 2x2 confusion matrix (rows: true HOLD / rotate,
    columns: predicted) and the per-epoch mean loss / accuracy."""
    t0 = time.time()
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    X, task_id = read_csv(data_path, N_OBS_PER_TRIAL * DIMS_PER_OBS)
    y = np.clip(task_id, 0, 1)
    train_idx, test_idx = train_test_split_indices(X.shape[0])
    if verbose:
        print("Fitting and scaling data")
    sc = fit_scaler(X[train_idx])
    X_train = torch.as_tensor((X[train_idx] - sc["mean_"]) / sc["scale_"], dtype=torch.float32).to(dev)
    X_test = torch.as_tensor((X[test_idx] - sc["mean_"]) / sc["scale_"], dtype=torch.float32).to(dev)
    y_train = torch.as_tensor(y[train_idx], dtype=torch.float32).to(dev)
    y_test = y[test_idx]

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        task_classifier = TaskClassifier()
    task_classifier.to(dev)
    if verbose:
        print(task_classifier)
    criterion = torch.nn.BCEWithLogitsLoss()
    optimizer = torch.optim.Adam(task_classifier.parameters(), lr=LEARNING_RATE)
    gen = torch.Generator().manual_seed(int(seed))
    # the reference's DataLoader(TrainData, batch_size=100, shuffle=True): the same index batches, gathered on the device
    loader = torch.utils.data.DataLoader(range(X_train.shape[0]), batch_size=BATCH_SIZE, shuffle=True, generator=gen)
    losses, accs = [], []
    task_classifier.train()
    for e in range(1, n_epochs + 1):
        epoch_loss = torch.zeros((), dtype=torch.float64, device=dev)
        epoch_acc = torch.zeros((), dtype=torch.float64, device=dev)
        for idx in loader:
            idx = idx.to(dev, non_blocking=True)
            X_batch, y_batch = X_train[idx], y_train[idx].unsqueeze(1)
            optimizer.zero_grad()
            y_pred = task_classifier(X_batch)
            loss = criterion(y_pred, y_batch)
            acc = binary_acc(y_pred, y_batch)
            loss.backward()
            optimizer.step()
            epoch_loss += loss.detach().to(torch.float64)        # python floats in the reference: float64 sums of fp32 values
            epoch_acc += acc.to(torch.float64)
        losses.append(epoch_loss / len(loader))
        accs.append(epoch_acc / len(loader))
        if verbose:
            print(f"Epoch {e + 0:03}: | Loss: {float(losses[-1]):.5f} | Accuracy: {float(accs[-1]):.3f}")
    losses = torch.stack(losses).cpu().numpy() if losses else np.zeros(0)
    accs = torch.stack(accs).cpu().numpy() if accs else np.zeros(0)
    t_train = time.time() - t0

    task_classifier.eval()
    with torch.no_grad():
        y_pred = torch.round(torch.sigmoid(task_classifier(X_test))).reshape(-1).cpu().numpy().astype(np.int64)
    cm = np.zeros((2, 2), dtype=np.int64)
    np.add.at(cm, (y_test, y_pred), 1)
    accuracy = float((y_pred == y_test).mean()) if len(y_test) else float("nan")
    if verbose:
        print(f"Test accuracy: {accuracy * 100:.2f} % on {len(y_test)} trials")
        print(f"Confusion matrix (rows: true hold / rotate, columns: predicted):\n{cm}")

    folder = save_folder if save_folder is not None else (os.path.dirname(os.path.abspath(data_path)))
    os.makedirs(folder, exist_ok=True)
    scaler_path, clf_path = os.path.join(folder, "scaler.pkl"), os.path.join(folder, "task_classifier.pt")
    save_scaler(scaler_path, sc)
    torch.save({k: v.detach().cpu() for k, v in task_classifier.state_dict().items()}, clf_path)
    return {"test_accuracy": accuracy, "confusion_matrix": cm, "epoch_losses": losses, "epoch_accuracies": accs,
            "n_train": int(len(train_idx)), "n_test": int(len(test_idx)), "train_seconds": t_train,
            "classifier_path": clf_path, "scaler_path": scaler_path}
