"""Datasets feeding the hot path.  PickleDataset reads the reference's on-disk format
({utt_id: {'feature': float32[T, D], 'token_ids': list[int]}}, dataset.py:46-80): length filter from the
config keys max/min_feature_length, max/min_text_length, keys sorted by frame count.
SyntheticDataset generates the same structure in memory for benchmarks and tests."""
import pickle

import numpy as np
from torch.utils.data import Dataset


def _shape0(feature):
    return feature.shape[0]


def _within(entry, config, frames_of=_shape0):
    frames = frames_of(entry["feature"])
    chars = len(entry["token_ids"])
    return (config["min_feature_length"] <= frames <= config["max_feature_length"]
            and config["min_text_length"] <= chars <= config["max_text_length"])


class DictDataset(Dataset):
    """Common behaviour over an {utt: {'feature', 'token_ids'}} dict.  `frames_of`: feature -> its frame count for the
    length filter and the sort (default: shape[0]; with a front end the features are waveforms and it is the front end's
    num_frames of the sample count)."""

    def __init__(self, data_dict, config=None, sort=True, frames_of=None):
        self.data_dict = data_dict
        frames_of = frames_of or _shape0
        keys = [k for k in data_dict if config is None or _within(data_dict[k], config, frames_of)]
        if sort:
            keys.sort(key=lambda k: frames_of(data_dict[k]["feature"]))
        self.keys = keys

    def __getitem__(self, index):
        item = self.data_dict[self.keys[index]]
        return item["feature"], item["token_ids"]

    def __len__(self):
        return len(self.keys)


class PickleDataset(DictDataset):
    def __init__(self, pickle_path, config=None, sort=True, frames_of=None):
        with open(pickle_path, "rb") as f:
            data = pickle.load(f)
        super().__init__(data, config=config, sort=sort, frames_of=frames_of)


def synthetic_utterances(n, input_dim, vocab_size, t_max, seed, ragged=True, label_ratio=0.125):
    """N(0,1) features (CMVN-normalised fbank stand-in), lengths U[0.6 T, T] when ragged, labels
    uniform in [3, V), L = max(2, floor(label_ratio * T_i))."""
    rs = np.random.RandomState(seed)
    out = {}
    for i in range(n):
        t = int(rs.randint(int(0.6 * t_max), t_max + 1)) if ragged else int(t_max)
        out["utt%06d" % i] = dict(
            feature=rs.normal(0.0, 1.0, size=(t, input_dim)).astype(np.float32),
            token_ids=rs.randint(3, vocab_size, size=(max(2, int(label_ratio * t)),)).tolist())
    return out


def synthetic_waveforms(n, vocab_size, seconds_max, seed, sample_rate=16000, ragged=True, label_ratio=0.125,
                        frame_shift=160, dtype=np.int16):
    """Waveform stand-ins for synthetic_utterances: durations U[0.6 s, s] when ragged, two sines of random pitch under
    white noise at a random level, int16 (or float32 in int16 range); labels as there, from the utterance's frame count
    at `frame_shift` samples per frame."""
    rs = np.random.RandomState(seed)
    n_max = int(round(seconds_max * sample_rate))
    out = {}
    for i in range(n):
        m = int(rs.randint(int(0.6 * n_max), n_max + 1)) if ragged else n_max
        t = np.arange(m) / float(sample_rate)
        f1, f2 = rs.uniform(80.0, 400.0), rs.uniform(500.0, 0.45 * sample_rate)
        wave = rs.uniform(500.0, 8000.0) * (np.sin(2 * np.pi * f1 * t) + 0.5 * np.sin(2 * np.pi * f2 * t + rs.uniform(0, 6.28)))
        wave = np.clip(np.rint(wave + rs.normal(0.0, rs.uniform(50.0, 1000.0), m)), -32768, 32767)
        frames = max(1, m // frame_shift)
        out["utt%06d" % i] = dict(feature=wave.astype(dtype),
                                  token_ids=rs.randint(3, vocab_size, size=(max(2, int(label_ratio * frames)),)).tolist())
    return out


class SyntheticDataset(DictDataset):
    def __init__(self, n, input_dim, vocab_size, t_max, seed=1234, ragged=True, config=None, sort=True):
        super().__init__(synthetic_utterances(n, input_dim, vocab_size, t_max, seed, ragged), config=config,
                         sort=sort)
