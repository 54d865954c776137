"""Training driver with the reference Solver's surface (solver.py:13-565): same constructor, method
names, config keys, loss formulas and op order (zero_grad -> backward -> [all-reduce] -> clip -> step).
Differences, all MI355X-first: the optimiser is the fused flat-buffer FlatAdam (one HIP kernel for
clip+Adam(amsgrad)), gradients of a data-parallel run are exchanged with ONE RCCL all-reduce, and
under torch.distributed every rank draws the same global batch (identically seeded samplers), pads and uploads
only its strided shard - at the global extents (parallel.py), which reproduces the single-process numbers
exactly.  Batches reach HBM through feed.DeviceFeed: collated one step ahead into pinned memory and uploaded on
a side stream, so that the loops below never wait for a copy (the reference: to_gpu(data), utils.py:154-158).
"""
import math
import os
import pickle

import numpy as np
import torch

import hip_backend as hb
import ops
import parallel
from dataloader import get_data_loader, _raw_items, _raw_texts
from dataset import PickleDataset
from feed import DeviceFeed
from model import E2E, LM
from parallel import FlatAdam
from utils import (Logger, adjust_learning_rate, calculate_cer, calculate_cer_ids, calculate_wer_ids, cc, infinite_iter,
                   remove_pad_eos, to_sents)


class StepScalar(object):
    """A scalar of a train step (loss, ...) whose host copy may still be on its way: the step's kernels, its optimiser
    update included, are enqueued without waiting for it (Solver._step).  float() / format() / arithmetic resolve it -
    which waits for that step and deals with an abort latch it may carry.  Under data parallelism resolving a record may
    turn into a sequence of collectives (the coordinated repeat, parallel.DpPipeline._recover), so every rank has to
    resolve at the same points of its program: the Solver's loops do (they run the same code on all ranks); code of its own
    that reads a scalar on ONE rank only (a rank-0 log, a rank-0 save) calls Solver.flush() on EVERY rank first."""
    __slots__ = ("_rec", "_i")

    def __init__(self, rec, i):
        self._rec, self._i = rec, i

    def __float__(self):
        if self._rec["values"] is None:
            self._rec["resolve"](self._rec)
        return float(self._rec["values"][self._i])

    item = __float__

    def __format__(self, spec):
        return format(float(self), spec)

    def __repr__(self):
        return repr(float(self))

    def __reduce__(self):                               # pickles (torch.save of a log) as the plain float
        return (float, (float(self),))


def _float_op(name):
    def op(self, *args):
        return getattr(float(self), name)(*[float(a) if isinstance(a, StepScalar) else a for a in args])
    return op


for _name in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__", "__neg__",
              "__abs__", "__lt__", "__le__", "__gt__", "__ge__", "__eq__", "__ne__", "__pow__", "__bool__"):
    setattr(StepScalar, _name, _float_op(_name))
StepScalar.__hash__ = lambda self: hash(float(self))


class Solver(object):
    def __init__(self, config, load_model=False):
        self.config = config
        # `frontend` (not a reference key; absent by default): the datasets hold 1-D waveforms and the features are computed
        # on the GPU (frontend.Frontend); absent, the datasets hold feature matrices as in the reference
        self.frontend = None
        if config.get("frontend") is not None:
            from frontend import Frontend
            self.frontend = Frontend(config["frontend"])
            if int(config["input_dim"]) != self.frontend.output_dim:
                raise ValueError("config: input_dim %d, but the front end gives %d features per frame (n_mels %d x (1 + "
                                 "delta_order %d))" % (int(config["input_dim"]), self.frontend.output_dim,
                                                       self.frontend.n_mels, self.frontend.delta_order))
        self._paths_reported = False
        self._pending = []                 # train steps whose host read (scalars + abort latch) is outstanding, oldest first
        self._pinned = None                # their landing slots in pinned host memory
        self._dp_pipe = None               # the same for data-parallel steps (parallel.DpPipeline)
        self.rank, self.world, _ = parallel.init_distributed()
        # The reference never seeds numpy (teacher-forcing draws model.py:328, input noise solver.py:370-373).  Data-parallel
        # ranks must draw identical streams, so `numpy_seed` (not a reference key) defaults to 0 there;
        # a single process stays unseeded like the reference unless the key is given.
        seed = config.get("numpy_seed", 0 if self.world > 1 else None)
        if seed is not None:
            np.random.seed(int(seed))
        if self.rank == 0:
            print(self.config)
        self.logger = Logger(config["logdir"])
        self.load_vocab()
        self.mwer_space = self.mwer_unit_config(config, self.vocab)
        self.get_data_loaders()
        self.labeldist = self.get_label_dist(self.train_lab_dataset)
        self.unlab_labeldist = self.get_label_dist(self.train_unlab_y_dataset)
        self.proportion = self.calculate_length_proportion()
        self.build_model(load_model=load_model)
        self.model.space_id = self.mwer_space      # E2E.mwer_forward(unit="word") splits the hypotheses at this id
        # the pseudo-labelling keys are refused here where they cannot hold; absent, nothing differs
        self.pseudo_config(config, self.world, hasattr(self.model, "ctc_lo"))
        self.settle_host_memory()         # the corpora stay for good: keep the garbage collector from walking them mid-epoch

    # ------------------------------------------------------------------ checkpoints (.ckpt/.opt/.judge.*)
    def save_model(self, model_path):
        self.flush()
        if self.rank == 0:
            torch.save(self.model.state_dict(), f"{model_path}.ckpt")
            torch.save(self.gen_opt.state_dict(), f"{model_path}.opt")

    def save_judge(self, model_path):
        self.flush()
        if self.rank == 0:
            torch.save(self.judge.state_dict(), f"{model_path}.judge.ckpt")
            torch.save(self.dis_opt.state_dict(), f"{model_path}.judge.opt")

    def load_model(self, model_path, load_optimizer):
        print(f"Load model from {model_path}.ckpt")
        state = torch.load(f"{model_path}.ckpt", map_location="cpu")
        head = [k for k in self.model.state_dict() if k.startswith("ctc_lo.")]
        headless = bool(head) and not any(k in state for k in head)
        if headless:
            # an attention-only checkpoint into a model with the CTC branch (`ctc_weight` > 0): everything else loads, the
            # head keeps its initialisation
            if self.rank == 0:
                print(f"{model_path}.ckpt has no CTC head ({', '.join(head)}): the head keeps its initialisation")
            state = dict(state, **{k: v for k, v in self.model.state_dict().items() if k in head})
        # the transducer head follows the same rule (`rnnt_weight` > 0): a checkpoint without it loads, the head keeps its
        # initialisation; the optimiser state of such a run cannot be resumed
        rnnt_head = [k for k in self.model.state_dict() if k.startswith("rnnt.")]
        rnnt_headless = bool(rnnt_head) and not any(k in state for k in rnnt_head)
        if rnnt_headless:
            if self.rank == 0:
                print(f"{model_path}.ckpt has no transducer head (rnnt.*): the head keeps its initialisation")
            state = dict(state, **{k: v for k, v in self.model.state_dict().items() if k in rnnt_head})
        self.model.load_state_dict(state)
        if load_optimizer:
            if rnnt_headless:
                raise RuntimeError(f"{model_path}.opt belongs to a model without the transducer head: its optimiser state "
                                   "cannot be resumed with `rnnt_weight` > 0 (set load_optimizer: false)")
            if headless:
                raise RuntimeError(f"{model_path}.opt belongs to a model without the CTC head: the optimiser state of an "
                                   "attention-only run cannot be resumed with `ctc_weight` > 0 (set load_optimizer: false)")
            print(f"Load optmizer from {model_path}.opt")
            self.gen_opt.load_state_dict(torch.load(f"{model_path}.opt", map_location="cpu"))

    def load_judge(self, model_path, load_optimizer):
        self.judge.load_state_dict(torch.load(f"{model_path}.judge.ckpt", map_location="cpu"))
        if load_optimizer:
            self.dis_opt.load_state_dict(torch.load(f"{model_path}.judge.opt", map_location="cpu"))

    # ------------------------------------------------------------------ data
    def load_vocab(self):
        with open(self.config["vocab_path"], "rb") as f:
            self.vocab = pickle.load(f)
        with open(self.config["non_lang_syms_path"], "rb") as f:
            self.non_lang_syms = pickle.load(f)

    def get_label_dist(self, dataset):
        counts = np.zeros(len(self.vocab))
        for _, tokens in dataset:
            np.add.at(counts, np.asarray(tokens, dtype=np.int64), 1.0)
        counts[self.vocab["<EOS>"]] += len(dataset)
        counts[self.vocab["<PAD>"]] = 0
        counts[self.vocab["<BOS>"]] = 0
        return counts / counts.sum()

    def calculate_length_proportion(self):
        frames_of = self.frontend.frames_of if self.frontend is not None else (lambda x: x.shape[0])
        frames = sum(frames_of(x) for x, _ in self.train_lab_dataset)
        chars = sum(len(y) for _, y in self.train_lab_dataset)
        return chars / frames

    def _dataset(self, name, config, sort=True):
        return PickleDataset(os.path.join(self.config["dataset_root_dir"], f"{name}.pkl"), config=config, sort=sort,
                             frames_of=self.frontend.frames_of if self.frontend is not None else None)

    def _loader(self, dataset, batch_size, shuffle, drop_last, **kw):
        # every rank must draw the SAME global batches: seed the sampler identically
        gen = torch.Generator()
        gen.manual_seed(int(self.config.get("data_seed", 0)))
        return get_data_loader(dataset, batch_size=batch_size, shuffle=shuffle, drop_last=drop_last, generator=gen,
                               **kw)

    def get_data_loaders(self):
        cfg = self.config
        bs, shuffle = cfg["batch_size"] * self.world, cfg["shuffle"]     # batch_size is per GPU
        bucket = bool(cfg.get("bucket_batches", False))     # not a reference key: length-bucketed speech batches
        self.train_lab_dataset = self._dataset(cfg["labeled_set"], cfg)
        self.train_lab_loader = self._loader(self.train_lab_dataset, bs, shuffle, False, bucket=bucket)
        self.train_unlab_x_dataset = self._dataset(cfg["unlabeled_speech_set"], cfg)
        self.train_unlab_x_loader = self._loader(self.train_unlab_x_dataset, bs, shuffle, False, speech_only=True,
                                                 bucket=bucket)
        self.train_unlab_y_dataset = self._dataset(cfg["unlabeled_text_set"], cfg)
        self.train_unlab_y_loader = self._loader(self.train_unlab_y_dataset, bs, shuffle, True, text_only=True)
        self.dev_dataset = self._dataset(cfg["dev_set"], None)
        self.dev_loader = self._loader(self.dev_dataset, cfg["batch_size"] // 2, False, False)

    def _feed(self, loader, kind="labeled", sharded=True, noise_std=0.0, endless=False, train=False):
        """The device-side view of a loader: the same batches in the same order (the loader's own batch sampler), collated
        one step ahead into pinned memory and uploaded on a side stream (feed.DeviceFeed) - this rank's strided rows only
        when `sharded` and the run is data parallel.  Config keys (not reference keys): `prefetch_batches` (default 2),
        `prefetch_thread` (default true: collate in a background thread)."""
        from torch.utils.data import DataLoader
        # (the loader's generator too: iterating a DataLoader draws a base seed from it before the sampler draws its
        # permutation - the batches are then the ones `for data in loader` would have produced)
        raw = DataLoader(loader.dataset, batch_sampler=loader.batch_sampler, num_workers=0, generator=loader.generator,
                         collate_fn=_raw_texts if kind == "text" else _raw_items)
        rank, world = (self.rank, self.world) if sharded else (0, 1)
        return DeviceFeed(infinite_iter(raw) if endless else raw, "cuda" if torch.cuda.is_available() else "cpu", kind=kind,
                          rank=rank, world=world, depth=int(self.config.get("prefetch_batches", 2)), noise_std=noise_std,
                          thread=bool(self.config.get("prefetch_thread", True)), frontend=self.frontend, train=train)

    def get_infinite_iter(self):
        self.lab_iter = iter(self._feed(self.train_lab_loader, endless=True, train=True))
        self.unlab_x_iter = iter(self._feed(self.train_unlab_x_loader, kind="speech", endless=True, train=True))
        self.unlab_y_iter = iter(self._feed(self.train_unlab_y_loader, kind="text", endless=True))

    # ------------------------------------------------------------------ model + optimisers
    def build_model(self, load_model=False):
        cfg = self.config
        self.model = cc(E2E(
            input_dim=cfg["input_dim"], enc_hidden_dim=cfg["enc_hidden_dim"], enc_n_layers=cfg["enc_n_layers"],
            subsample=cfg["subsample"], dropout_rate=cfg["dropout_rate"], dec_hidden_dim=cfg["dec_hidden_dim"],
            att_dim=cfg["att_dim"], conv_channels=cfg["conv_channels"], conv_kernel_size=cfg["conv_kernel_size"],
            att_odim=cfg["att_odim"], output_dim=len(self.vocab), embedding_dim=cfg["embedding_dim"],
            ls_weight=cfg["ls_weight"], labeldist=self.labeldist, pad=self.vocab["<PAD>"], bos=self.vocab["<BOS>"],
            eos=self.vocab["<EOS>"],
            # `ctc_weight` (not a reference key; default 0): w > 0 adds the CTC branch on the encoder and every labeled
            # step trains on (1 - w) L_att + w L_ctc; at 0 the model is the reference's
            ctc_weight=float(cfg.get("ctc_weight", 0.0)),
            # `ctc_star_penalty` (not a reference key; absent or null = off): a float <= 0 makes the CTC term of every
            # training step the star CTC loss, for transcripts with missing words; it needs ctc_weight > 0
            ctc_star_penalty=cfg.get("ctc_star_penalty", None),
            # `rnnt_weight`, `rnnt_joint_dim`, `rnnt_pred_dim` (not reference keys; absent by default): w > 0 adds the
            # transducer head and the term w L_rnnt; the keys reach the model only then
            **self.rnnt_model_args(cfg)))
        # `dp_overlap` (not a reference key): issue the gradient all-reduce in buckets from inside the backward pass
        # (parallel.FlatBuffers.enable_overlap).  Off by default HERE: an RCCL kernel that is resident while a persistent
        # kernel is being placed could - if the two do not fit a CU together and a rank is late - hold that kernel's
        # workgroups back until its bounded spins expire (every rank then repeats the step off the persistent kernels).
        # bench.py measures it as a labelled sub-object; turn it on here once a multi-GPU run has shown the latch stays clear.
        overlap = bool(cfg.get("dp_overlap", False))
        # `deterministic` (not a reference key; default false, env ASR_DETERMINISTIC=1): every train step of this Solver runs
        # in hip_backend's deterministic mode - ordered reductions in place of the fp32 atomics, no side stream:
        # two runs from the same state and seeds give the same bits.  One process; with several ranks it covers each rank's
        # own computation, not the collective.  The bucketed exchange reads gradients from inside the backward pass: refused.
        self.deterministic = bool(cfg.get("deterministic", hb.DETERMINISTIC[0]))
        if self.deterministic and overlap:
            raise ValueError("`deterministic` and `dp_overlap` exclude each other: the bucketed all-reduce is issued from "
                             "inside the backward pass, in an order of its own")
        # `persist_retry_steps` (not a reference key): train steps on the per-step kernels after an abort of the persistent
        # ones before they are tried again (hip_backend.PERSIST_RETRY_STEPS: 200, doubling per abort; 0: never)
        if "persist_retry_steps" in cfg:
            hb.PERSIST_RETRY_STEPS = int(cfg["persist_retry_steps"])
        self.gen_opt = FlatAdam(self.model, lr=cfg["learning_rate"], weight_decay=cfg["weight_decay"], amsgrad=True,
                                max_grad_norm=cfg["max_grad_norm"], overlap=overlap)
        if load_model:
            self.load_model(cfg["load_model_path"], cfg["load_optimizer"])
        self.judge = cc(LM(
            output_dim=len(self.vocab), embedding_dim=cfg["dis_embedding_dim"], hidden_dim=cfg["dis_hidden_dim"],
            dropout_rate=cfg["dis_dropout_rate"], n_layers=cfg["dis_layers"], bos=self.vocab["<BOS>"],
            eos=self.vocab["<EOS>"], pad=self.vocab["<PAD>"], ls_weight=cfg["ls_weight"],
            labeldist=self.unlab_labeldist))
        self.dis_opt = FlatAdam(self.judge, lr=cfg["d_learning_rate"], max_grad_norm=cfg["max_grad_norm"], overlap=overlap)
        if self.rank == 0:
            print(self.model)
            print(self.judge)

    # ------------------------------------------------------------------ text scoring
    def _cer_device(self):
        """The device that scores CER when `cer_on_gpu` (not a reference key; default false) is set and the model is on a
        GPU: one launch of the edit-distance kernel over the whole set (utils.calculate_cer_ids) instead of the host's
        Levenshtein loop per utterance; None: the host loop."""
        dev = next(self.model.parameters()).device
        return dev if self.config.get("cer_on_gpu", False) and dev.type == "cuda" else None

    def _wer_device(self):
        """The device that scores WER when `wer_on_gpu` (not a reference key; default false) is set and the model is on a GPU
        (utils.calculate_wer_ids); None: Solver.test reports no WER.  Independent of `cer_on_gpu`."""
        dev = next(self.model.parameters()).device
        return dev if self.config.get("wer_on_gpu", False) and dev.type == "cuda" else None

    def _score_ids(self, hyp_ids, ref_ids, ref_index=None):
        return calculate_cer_ids(hyp_ids, ref_ids, self.vocab, self.non_lang_syms, self.vocab["<EOS>"], self._cer_device(),
                                 ref_index=ref_index)

    def ind2sent(self, all_prediction, all_ys):
        hyp_ids = remove_pad_eos(all_prediction, eos=self.vocab["<EOS>"])
        hyps = to_sents(hyp_ids, self.vocab, self.non_lang_syms)
        refs = to_sents(all_ys, self.vocab, self.non_lang_syms)
        if self._cer_device() is not None:
            return self._score_ids(hyp_ids, all_ys)[0], hyps, refs
        return calculate_cer(hyps, refs), hyps, refs

    def _abort_seen(self, dev):
        """True if a persistent kernel aborted on ANY rank since the latch was last cleared (synchronises).  Under data
        parallelism the decision is collective (all-reduce MAX of the latch), so that all ranks leave the persistent
        kernels together or none does - ranks on different kernel paths would still compute the same numbers, but a rank
        that alone repeats a batch must not be the one the others wait for in the next collective."""
        if dev.type != "cuda":
            return False
        flag = hb.persist_abort_flag(dev)[:1].float().clone()
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return flag.item() != 0.0

    def _greedy(self, xs, ilens):
        """Greedy hypothesis ids for one batch.  No loss is read on this path, so the abort word of the persistent
        kernels is checked explicitly after the decode (the copy to the host has synchronised anyway): an aborted
        launch poisons its outputs, which would otherwise surface as a silently wrong CER.  On an abort this process
        switches to the per-step kernels and decodes the batch again, as _backward_guarded does for a train step."""
        def run():
            with torch.no_grad():
                _, _, prediction, _ = self.model(xs, ilens, ys=None, max_dec_timesteps=self.config["max_dec_timesteps"])
            return prediction.cpu().numpy().tolist()
        out = run()
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during greedy decoding (this rank's code %d): repeating the batch on the "
                  "per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = run()
        return out

    ATT_NGRAM_LM_KEYS = ("arpa", "weight", "bonus")
    ATT_WORD_LM_KEYS = ("arpa", "lexicon", "weight", "bonus", "lexicon_only")

    @staticmethod
    def att_lm_config(config):
        """`att_ngram_lm` and `att_word_lm` (not reference keys; absent by default): the n-gram LM, or the lexicon
        and the word-level LM, INSIDE the attention beam search (E2E.recognize_beams) - sub-dictionaries in the style of
        `rnnt_word_lm`: `att_ngram_lm: {arpa, weight, bonus}` (an ARPA file over the vocabulary's symbols; bonus per token) and
        `att_word_lm: {arpa, lexicon, weight, bonus, lexicon_only}` (an ARPA file over words spelled in the vocabulary's
        characters, an optional lexicon file; bonus per completed word).  They combine with `lm_weight` and
        `ctc_decode_weight`.  -> (kind, the sub-dictionary) with kind "ngram" / "word", or (None, None); ValueError with both,
        without `beam_size` > 1, beside another decoder's key, without `arpa`, or with a sub-key that is none of these."""
        ng, wd = config.get("att_ngram_lm"), config.get("att_word_lm")
        if ng is None and wd is None:
            return None, None
        if ng is not None and wd is not None:
            raise ValueError("att_ngram_lm and att_word_lm are two LMs for one search: set one of them")
        name, sub, keys = ("att_ngram_lm", ng, Solver.ATT_NGRAM_LM_KEYS) if ng is not None else \
            ("att_word_lm", wd, Solver.ATT_WORD_LM_KEYS)
        others = [k for k in ("rnnt_beam_decode", "rnnt_greedy_decode", "two_pass_decode", "ctc_beam_decode", "ctc_greedy_decode")
                  if config.get(k)]
        if others:
            raise ValueError("%s is the LM of the attention beam search: it does not combine with %s" % (name, ", ".join(others)))
        if int(config.get("beam_size", 1) or 1) <= 1:
            raise ValueError("%s is the LM of the attention beam search: set beam_size > 1" % name)
        unknown = sorted(set(sub) - set(keys)) if isinstance(sub, dict) else None
        if unknown is None or unknown or not sub.get("arpa"):
            raise ValueError("%s is a dictionary with `arpa` and optionally %s%s"
                             % (name, ", ".join(keys[1:]), "; got %s" % ", ".join(unknown) if unknown else ""))
        return ("ngram" if ng is not None else "word"), sub

    def _beam(self, xs, ilens, beam_size, lm_weight=0.0, nbest=False, ctc_decode_weight=0.0, table_lm=None):
        """Best beam-search hypothesis ids for one batch (E2E.recognize_beams; lm_weight > 0: rescored by the judge, shallow
        fusion; table_lm: the keyword arguments of an n-gram or word LM inside the search) - with nbest all
        beam_size of them per utterance, ranked ([B][K][L]).  The encoder still runs on the
        persistent LSTM kernels: the abort word is checked after the decode and the batch repeated on the per-step kernels,
        as in _greedy."""
        def run():
            prediction, _ = self.model.recognize_beams(
                xs, ilens, self.config["max_dec_timesteps"], beam_size,
                length_penalty=float(self.config.get("beam_length_penalty", 0.0)), nbest=nbest,
                lm=self.judge if lm_weight > 0 else None, lm_weight=lm_weight,
                **(dict(ctc_decode_weight=ctc_decode_weight) if ctc_decode_weight > 0 else {}), **(table_lm or {}))
            return prediction.cpu().numpy().tolist()
        out = run()
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during beam decoding (this rank's code %d): repeating the batch on the "
                  "per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = run()
        return out

    @staticmethod
    def rnnt_model_args(config):
        """The transducer keys of the model (not reference keys; absent by default): `rnnt_weight` in [0, 1]
        (with `ctc_weight` at most 1 in sum), `rnnt_joint_dim` (default 256, a multiple of 4), `rnnt_pred_dim` (default: the
        decoder's width) -> the keyword arguments of E2E; none at weight 0, whatever the other two say."""
        w = float(config.get("rnnt_weight", 0.0) or 0.0)
        if not 0.0 <= w <= 1.0 or w + float(config.get("ctc_weight", 0.0) or 0.0) > 1.0:
            raise ValueError("rnnt_weight must lie in [0, 1] and ctc_weight + rnnt_weight must be at most 1")
        if w == 0:
            return {}
        return dict(rnnt_weight=w, rnnt_joint_dim=int(config.get("rnnt_joint_dim", 256) or 256),
                    rnnt_pred_dim=config.get("rnnt_pred_dim", None))

    @staticmethod
    def rnnt_decode_config(config, has_rnnt_head):
        """`rnnt_greedy_decode` (not a reference key; default false): test() decodes with the transducer head alone
        (E2E.recognize_rnnt, at most `rnnt_max_symbols` - default 3 - tokens per encoder frame).  It is a decoder of its own
        -> the key as a bool; ValueError on a model without the head or beside any other decoder or LM key."""
        on = bool(config.get("rnnt_greedy_decode", False))
        if not on:
            return False
        if not has_rnnt_head:
            raise ValueError("rnnt_greedy_decode needs the transducer head: build the model with rnnt_weight > 0")
        others = [k for k in ("two_pass_decode", "ctc_beam_decode", "ctc_greedy_decode", "ngram_lm", "word_lm") if config.get(k)]
        if int(config.get("beam_size", 1) or 1) > 1:
            others.append("beam_size > 1")
        others += [k + " > 0" for k in ("lm_weight", "ctc_decode_weight") if float(config.get(k, 0.0) or 0.0) > 0]
        if others:
            raise ValueError("rnnt_greedy_decode decodes with the transducer head alone: it does not combine with %s"
                             % ", ".join(others))
        return True

    @staticmethod
    def rnnt_beam_config(config, has_rnnt_head):
        """`rnnt_beam_decode` (not a reference key; default false): test() decodes with the transducer head's beam
        search (E2E.recognize_rnnt_beams, beam width `beam_size`, at most `max_dec_timesteps` labels), with `ngram_lm` inside
        it when that is set (`ngram_weight`, `ngram_bonus`).  It is a decoder of its own -> the key as a bool; ValueError on a
        model without the head or beside any other decoder's key, `word_lm` or `lm_weight`.
        `rnnt_word_lm` is this search's word-level LM, a sub-dictionary in the style of `frontend`: `arpa` (the
        path of an ARPA file over words spelled in the vocabulary's characters), `lexicon` (an optional path, one word per
        line), `weight`, `bonus` (per completed word), `lexicon_only`.  ValueError without `rnnt_beam_decode`, beside
        `ngram_lm`, without `arpa` or with a key that is none of these."""
        wlm = config.get("rnnt_word_lm")
        if not bool(config.get("rnnt_beam_decode", False)):
            if wlm is not None:
                raise ValueError("rnnt_word_lm is the word LM of the transducer beam search: set rnnt_beam_decode")
            return False
        if not has_rnnt_head:
            raise ValueError("rnnt_beam_decode needs the transducer head: build the model with rnnt_weight > 0")
        others = [k for k in ("rnnt_greedy_decode", "two_pass_decode", "ctc_beam_decode", "ctc_greedy_decode", "word_lm")
                  if config.get(k)]
        others += [k + " > 0" for k in ("lm_weight", "ctc_decode_weight") if float(config.get(k, 0.0) or 0.0) > 0]
        if others:
            raise ValueError("rnnt_beam_decode decodes with the transducer head alone: it does not combine with %s "
                             "(ngram_lm is the LM of this search)" % ", ".join(others))
        if config.get("ngram_lm") is None:
            for key in ("ngram_weight", "ngram_bonus"):
                if key in config:
                    raise ValueError("%s is set without ngram_lm, the ARPA file it weighs" % key)
        if wlm is not None:
            if config.get("ngram_lm") is not None:
                raise ValueError("rnnt_word_lm and ngram_lm are two LMs for one search: set one of them")
            unknown = sorted(set(wlm) - set(Solver.RNNT_WORD_LM_KEYS)) if isinstance(wlm, dict) else None
            if unknown is None or unknown or not wlm.get("arpa"):
                raise ValueError("rnnt_word_lm is a dictionary with `arpa` and optionally %s%s"
                                 % (", ".join(Solver.RNNT_WORD_LM_KEYS[1:]), "; got %s" % ", ".join(unknown) if unknown else ""))
        return True

    RNNT_WORD_LM_KEYS = ("arpa", "lexicon", "weight", "bonus", "lexicon_only")

    def _rnnt_beams(self, xs, ilens, beam_size, ngram=None, nbest=False):
        """Hypothesis ids of the transducer beam search for one batch (E2E.recognize_rnnt_beams, with the n-gram LM - or, ngram
        being the keyword arguments of a word LM, the lexicon and the word LM - inside when there is one) - with nbest beam_size id lists per utterance, ranked, a rank the search left unused as a row of
        <EOS>; the abort word of the encoder's persistent kernels is checked after the decode, as in _greedy."""
        kw = dict(max_dec_timesteps=int(self.config.get("max_dec_timesteps", 200) or 200), **self._lm_kwargs(ngram))

        def run():
            ids = self.model.recognize_rnnt_beams(xs, ilens, beam_size, **kw)
            if not nbest:
                return ids
            last = self.model.last_rnnt_beams
            eos = self.vocab["<EOS>"]
            rows = torch.cat([last["lengths"].unsqueeze(2), last["tokens"]], dim=2).cpu().tolist()
            hyps = [[r[1:1 + max(r[0], 0)] for r in utt] for utt in rows]
            width = max(len(h) for utt in hyps for h in utt) + 1
            return [[h + [eos] * (width - len(h)) for h in utt] for utt in hyps]
        out = run()
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during transducer beam decoding (this rank's code %d): repeating the batch on "
                  "the per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = run()
        return out

    def _rnnt_greedy(self, xs, ilens):
        """Greedy hypothesis ids of the transducer head for one batch (E2E.recognize_rnnt); the abort word of the encoder's
        persistent kernels is checked after the decode and the batch repeated on the per-step kernels, as in _greedy."""
        kw = dict(max_symbols=int(self.config.get("rnnt_max_symbols", 3) or 3),
                  max_dec_timesteps=int(self.config.get("max_dec_timesteps", 200) or 200))
        out = self.model.recognize_rnnt(xs, ilens, **kw)
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during transducer decoding (this rank's code %d): repeating the batch on the "
                  "per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = self.model.recognize_rnnt(xs, ilens, **kw)
        return out

    def _ctc_best_path(self, xs, ilens):
        """Best-path hypothesis ids of the CTC head for one batch (E2E.recognize_ctc); the abort word of the encoder's
        persistent kernels is checked after the decode and the batch repeated on the per-step kernels, as in _greedy."""
        out = self.model.recognize_ctc(xs, ilens)
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during CTC best-path decoding (this rank's code %d): repeating the batch on "
                  "the per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = self.model.recognize_ctc(xs, ilens)
        return out

    @staticmethod
    def two_pass_config(config, has_ctc_head):
        """`two_pass_decode` (not a reference key; default false): test() decodes with E2E.recognize_two_pass -
        the CTC prefix beam search proposes `beam_size` hypotheses, the attention decoder (and with `lm_weight` > 0 the judge)
        rescores them in one teacher-forced pass; `ctc_decode_weight` is the CTC score's weight in the combination.  -> the
        key as a bool; ValueError where it cannot hold: together with `ctc_greedy_decode` (a decoder of its own), or on a model
        without the CTC head."""
        on = bool(config.get("two_pass_decode", False))
        if on and bool(config.get("ctc_greedy_decode", False)):
            raise ValueError("two_pass_decode and ctc_greedy_decode are two decoders: set one of them")
        if on and not has_ctc_head:
            raise ValueError("two_pass_decode needs the CTC head: build the model with ctc_weight > 0")
        return on

    @staticmethod
    def ngram_config(config, two_pass, has_ctc_head):
        """The n-gram LM keys (not reference keys; absent by default): `ctc_beam_decode` (default false) makes
        test() decode with the CTC prefix beam search alone (E2E.recognize_ctc_beams, beam width `beam_size`); `ngram_lm` is
        the path of an ARPA file over the vocabulary's symbols, used inside that search with `ctc_beam_decode` and inside
        the first pass (and the combination) with `two_pass_decode`; `ngram_weight` and `ngram_bonus` weigh its
        log-probability and the hypothesis length.  -> (ctc_beam_decode as a bool, the path or None, weight, bonus);
        ValueError where the keys cannot hold: `ctc_beam_decode` beside another decoder or on a model without the CTC head,
        `ngram_lm` with a decoder that has no place for it, a weight or bonus without `ngram_lm`."""
        ctc_beam = bool(config.get("ctc_beam_decode", False))
        if ctc_beam and (two_pass or bool(config.get("ctc_greedy_decode", False))):
            raise ValueError("ctc_beam_decode, two_pass_decode and ctc_greedy_decode are three decoders: set one of them")
        if ctc_beam and not has_ctc_head:
            raise ValueError("ctc_beam_decode needs the CTC head: build the model with ctc_weight > 0")
        if ctc_beam and (float(config.get("lm_weight", 0.0) or 0.0) > 0 or float(config.get("ctc_decode_weight", 0.0) or 0.0) > 0):
            raise ValueError("ctc_beam_decode decodes with the CTC head alone: it does not combine with lm_weight > 0 or "
                             "ctc_decode_weight > 0 (ngram_lm is the LM of this search)")
        path = config.get("ngram_lm")
        if path is None:
            for key in ("ngram_weight", "ngram_bonus"):
                if key in config:
                    raise ValueError("%s is set without ngram_lm, the ARPA file it weighs" % key)
            return ctc_beam, None, 0.0, 0.0
        if not (ctc_beam or two_pass):
            raise ValueError("ngram_lm is used by the CTC prefix beam search: set ctc_beam_decode or two_pass_decode - the "
                             "attention beam search, greedy and ctc_greedy_decode have no place for an n-gram LM")
        return ctc_beam, path, float(config.get("ngram_weight", 0.0) or 0.0), float(config.get("ngram_bonus", 0.0) or 0.0)

    @staticmethod
    def word_lm_config(config, two_pass, ctc_beam):
        """The word LM keys (not reference keys; absent by default): `word_lm` is the path of an ARPA file over
        WORDS spelled in the vocabulary's characters, used with its lexicon inside the CTC prefix beam search
        (`ctc_beam_decode`) or the first pass and the combination of `two_pass_decode`; `lexicon` an optional path, one word
        per line (default: the ARPA unigrams); `word_lm_weight` and `word_bonus` weigh its log-probability and the number of
        words; `lexicon_only` keeps only sequences of lexicon words.  -> (path or None, lexicon path or None, weight,
        bonus, lexicon_only).  ValueError: `word_lm` with any other decoder or beside `ngram_lm`, another of the keys
        without `word_lm`."""
        path = config.get("word_lm")
        if path is None:
            for key in ("lexicon", "word_lm_weight", "word_bonus", "lexicon_only"):
                if config.get(key):
                    raise ValueError("%s is set without word_lm, the ARPA file it goes with" % key)
            return None, None, 0.0, 0.0, False
        if config.get("ngram_lm") is not None:
            raise ValueError("word_lm and ngram_lm are two LMs for one search: set one of them")
        if not (ctc_beam or two_pass):
            raise ValueError("word_lm is used by the CTC prefix beam search: set ctc_beam_decode or two_pass_decode - the "
                             "other decoders have no place for it")
        return path, config.get("lexicon"), float(config.get("word_lm_weight", 0.0) or 0.0), \
            float(config.get("word_bonus", 0.0) or 0.0), bool(config.get("lexicon_only", False))

    CONTEXT_BIAS_KEYS = ("phrases", "boost", "weight", "word_start_only")

    @staticmethod
    def context_config(config, two_pass, ctc_beam):
        """`context_bias` (not a reference key; absent by default): `{phrases, boost, weight, word_start_only}` -
        `phrases` the path of a file with one phrase per line in the vocabulary's symbols and an optional trailing boost,
        `boost` the per-token boost of a line without one (default 1), `weight` what the bias is weighed by in the rank
        (default 1), `word_start_only` (default false) lets a phrase begin only at the start or behind <space>.  The list
        sits inside the CTC prefix beam search (`ctc_beam_decode`) or the first pass and the combination of
        `two_pass_decode`, alone or beside `ngram_lm`.  -> the sub-dictionary or None.  ValueError: with any other decoder,
        beside `word_lm`, without `phrases` or with a key that is none of these."""
        sub = config.get("context_bias")
        if sub is None:
            return None
        if not isinstance(sub, dict) or not sub.get("phrases"):
            raise ValueError("context_bias is a dictionary {phrases: <file>, boost, weight, word_start_only} with phrases set")
        unknown = [k for k in sub if k not in Solver.CONTEXT_BIAS_KEYS]
        if unknown:
            raise ValueError("context_bias: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(Solver.CONTEXT_BIAS_KEYS)))
        if not (ctc_beam or two_pass):
            raise ValueError("context_bias is used by the CTC prefix beam search: set ctc_beam_decode or two_pass_decode - the "
                             "other decoders have no place for it")
        if config.get("word_lm") is not None:
            raise ValueError("context_bias beside word_lm is not built: use it alone or with ngram_lm")
        return sub

    def load_context(self, sub):
        """The ContextGraph of a `context_bias` dictionary over this vocabulary's symbols."""
        from context import ContextGraph
        space = None
        if sub.get("word_start_only"):
            if "<space>" not in self.vocab:
                raise ValueError("context_bias: word_start_only needs <space> in the vocabulary")
            space = self.vocab["<space>"]
        return ContextGraph.from_text(sub["phrases"], self.vocab, boost=float(sub.get("boost", 1.0) or 1.0), V=len(self.vocab),
                                      word_start_only=space)

    def load_word_lm(self, path, lexicon_path=None):
        """The WordLM of an ARPA file over words spelled in this vocabulary's one-character symbols, split at <space>."""
        from word_lm import WordLM
        if "<space>" not in self.vocab:
            raise ValueError("word_lm needs <space> in the vocabulary: words are what lies between two of them")
        lexicon = None
        if lexicon_path is not None:
            with open(lexicon_path, "r", encoding="utf-8") as f:
                lexicon = [line.split()[0] for line in f if line.strip()]
        chars = {s: i for s, i in self.vocab.items() if len(s) == 1}
        return WordLM.from_arpa(path, chars, self.vocab["<space>"], lexicon=lexicon, bos=self.vocab["<BOS>"],
                                eos=self.vocab["<EOS>"], V=len(self.vocab))

    def _ctc_beams(self, xs, ilens, beam_size, ngram=None, nbest=False):
        """Hypothesis ids of the CTC prefix beam search for one batch (E2E.recognize_ctc_beams, with the n-gram LM inside
        when there is one) - with nbest beam_size id lists per utterance, ranked, a rank the search left unused as a row
        of <EOS>; the abort word of the encoder's persistent kernels is checked after the decode, as in _greedy."""
        extra = self._lm_kwargs(ngram)

        def run():
            ids, _ = self.model.recognize_ctc_beams(xs, ilens, beam_size, nbest=nbest, **extra)
            if nbest:
                eos = self.vocab["<EOS>"]
                width = max(len(h) for hyps in ids for h in hyps) + 1
                ids = [[h + [eos] * (width - len(h)) for h in hyps + [[]] * (beam_size - len(hyps))] for hyps in ids]
            return ids
        out = run()
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during CTC beam decoding (this rank's code %d): repeating the batch on the "
                  "per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = run()
        return out

    @staticmethod
    def _lm_kwargs(ngram):
        """ngram: None, (the NgramLM, its weight, the length bonus), or the keyword arguments of a word LM as a dict."""
        if ngram is None:
            return {}
        if isinstance(ngram, dict):
            return ngram
        return dict(ngram=ngram[0], ngram_weight=ngram[1], ngram_bonus=ngram[2])

    def _two_pass(self, xs, ilens, beam_size, ctc_weight, lm_weight=0.0, nbest=False, ngram=None):
        """Two-pass hypothesis ids for one batch (E2E.recognize_two_pass) - with nbest all beam_size of them per utterance,
        ranked ([B][K][L]); the abort word of the persistent kernels is checked after the decode and the batch repeated on
        the per-step kernels, as in _greedy.  ngram: (the NgramLM, its weight, the length bonus) or None."""
        extra = self._lm_kwargs(ngram)

        def run():
            prediction, _ = self.model.recognize_two_pass(
                xs, ilens, beam_size, ctc_weight=ctc_weight,
                length_penalty=float(self.config.get("beam_length_penalty", 0.0)), nbest=nbest,
                lm=self.judge if lm_weight > 0 else None, lm_weight=lm_weight, **extra)
            return prediction.cpu().numpy().tolist()
        out = run()
        if self._abort_seen(xs.device):
            print("persistent kernels aborted during two-pass decoding (this rank's code %d): repeating the batch on the "
                  "per-step kernels" % hb.persist_abort_code(xs.device))
            hb.disable_persistent(xs.device)
            out = run()
        return out

    def align(self, loader=None):
        """CTC forced alignment of every utterance of `loader` (default: the dev loader) to its transcript with the model's
        CTC head (E2E.align; the model needs `ctc_weight` > 0) -> one record per utterance, in the loader's
        order: tokens (the vocabulary's symbols), first / last (inclusive encoder frames; times model.time_reduction for
        input frames), confidence (per token), score (the alignment's log-probability) and frames.  The device results are
        read once per batch."""
        self.flush()
        loader = self.dev_loader if loader is None else loader
        symbols = {i: s for s, i in self.vocab.items()}
        was_training = self.model.training
        self.model.eval()
        records = []
        try:
            for batch in self._feed(loader, sharded=False):
                xs, ilens, ys = batch
                out = self.model.align(xs, ilens, ys)
                if self._abort_seen(xs.device):                 # see _greedy
                    hb.disable_persistent(xs.device)
                    out = self.model.align(xs, ilens, ys)
                for rec in out:
                    rec["tokens"] = [symbols[i] for i in rec["tokens"]]
                records += out
        finally:
            self.model.train(was_training)
        return records

    def segment(self, loader_or_batches, min_confidence=None, window=30):
        """CTC segmentation of recordings against their transcripts with the model's CTC head (E2E.segment; the
        model needs `ctc_weight` > 0).  `loader_or_batches` yields (xs, ilens, texts) with `texts` a list, per recording, of
        label tensors, one per utterance.  -> one record per recording, in order: score, frames and utterances, each with
        tokens (the vocabulary's symbols), begin / end (inclusive encoder frames; times model.time_reduction for input
        frames), logp, confidence and keep (confidence >= min_confidence; True when no threshold is given).  The device
        results are read once per batch."""
        self.flush()
        symbols = {i: s for s, i in self.vocab.items()}
        was_training = self.model.training
        self.model.eval()
        records = []
        try:
            for xs, ilens, texts in loader_or_batches:
                out = self.model.segment(xs, ilens, texts, window=window)
                if self._abort_seen(xs.device):                 # see _greedy
                    hb.disable_persistent(xs.device)
                    out = self.model.segment(xs, ilens, texts, window=window)
                for rec in out:
                    for utt in rec["utterances"]:
                        utt["tokens"] = [symbols[i] for i in utt["tokens"]]
                        utt["keep"] = bool(min_confidence is None or utt["confidence"] >= min_confidence)
                records += out
        finally:
            self.model.train(was_training)
        return records

    def align_rnnt(self, loader=None):
        """Forced alignment of every utterance of `loader` (default: the dev loader) to its transcript with the model's
        transducer head (E2E.align_rnnt; the model needs `rnnt_weight` > 0) -> one record per utterance, in
        the loader's order: tokens (the vocabulary's symbols), frame (the encoder frame each token is emitted on; times
        model.time_reduction for input frames), confidence (per token), score (the alignment's log-probability) and frames.
        The device results are read once per batch."""
        self.flush()
        loader = self.dev_loader if loader is None else loader
        symbols = {i: s for s, i in self.vocab.items()}
        was_training = self.model.training
        self.model.eval()
        records = []
        try:
            for batch in self._feed(loader, sharded=False):
                xs, ilens, ys = batch
                out = self.model.align_rnnt(xs, ilens, ys)
                if self._abort_seen(xs.device):                 # see _greedy
                    hb.disable_persistent(xs.device)
                    out = self.model.align_rnnt(xs, ilens, ys)
                for rec in out:
                    rec["tokens"] = [symbols[i] for i in rec["tokens"]]
                records += out
        finally:
            self.model.train(was_training)
        return records

    def validation(self):
        """Teacher-forced dev loss + greedy CER (solver.py:212-242); greedy pass runs without autograd."""
        self.flush()
        self.model.eval()
        preds, refs, total, ctc_total, rnnt_total = [], [], 0.0, None, None
        for batch in self._feed(self.dev_loader, sharded=False):
            xs, ilens, ys = batch
            with torch.no_grad():
                _, log_probs, _, _ = self.model(xs, ilens, ys=ys)
                value = self.model.mask_and_cal_loss(log_probs, ys).item()
                if self._abort_seen(xs.device):             # the latch, not the loss: an abort need not reach the loss
                    hb.disable_persistent(xs.device)        # see _greedy
                    _, log_probs, _, _ = self.model(xs, ilens, ys=ys)
                    value = self.model.mask_and_cal_loss(log_probs, ys).item()
                total += value
                if getattr(log_probs, "ctc_loss", None) is not None:      # the CTC branch's own dev loss, per utterance
                    ctc_total = (ctc_total or 0.0) + log_probs.ctc_loss.item()
                if getattr(log_probs, "rnnt_loss", None) is not None:     # the transducer head's own dev loss, per utterance
                    rnnt_total = (rnnt_total or 0.0) + log_probs.rnnt_loss.item()
            preds += self._greedy(xs, ilens)
            refs += batch.ys_host
        self.model.train()
        # (the returned dev loss stays the attention loss, so that runs with and without the CTC branch compare)
        self.val_ctc_loss = None if ctc_total is None else ctc_total / len(self.dev_loader)
        if self.val_ctc_loss is not None:
            self._val_rounds = getattr(self, "_val_rounds", 0) + 1
            if self.rank == 0:
                print(f"val_ctc_loss={self.val_ctc_loss:.4f}")
            self.logger.scalar_summary(f"{self.config['tag']}/supervised/val_ctc_loss", self.val_ctc_loss, self._val_rounds - 1)
        self.val_rnnt_loss = None if rnnt_total is None else rnnt_total / len(self.dev_loader)
        if self.val_rnnt_loss is not None:
            self._val_rnnt_rounds = getattr(self, "_val_rnnt_rounds", 0) + 1
            if self.rank == 0:
                print(f"val_rnnt_loss={self.val_rnnt_loss:.4f}")
            self.logger.scalar_summary(f"{self.config['tag']}/supervised/val_rnnt_loss", self.val_rnnt_loss,
                                       self._val_rnnt_rounds - 1)
        cer, hyp_sents, ref_sents = self.ind2sent(preds, refs)
        return total / len(self.dev_loader), cer, hyp_sents, ref_sents

    def lm_validation(self):
        self.flush()
        self.judge.eval()
        total = 0.0
        for batch in self._feed(self.dev_loader, kind="text", sharded=False):     # transcripts, longest first
            ys = list(batch)
            with torch.no_grad():
                log_probs, _, _ = self.judge(ys)
                value = -self.judge.mask_and_cal_sum(log_probs, ys).item()
                if ys and self._abort_seen(ys[0].device):   # the H = 640 judge runs on the persistent kernels too: a latch
                    hb.disable_persistent(ys[0].device)     # left here would fail the next (clean) training step
                    log_probs, _, _ = self.judge(ys)
                    value = -self.judge.mask_and_cal_sum(log_probs, ys).item()
                total += value
        samples = self.judge.decode(n_samples=5, sample=True,
                                    max_dec_timesteps=int(self.config.get("lm_sample_steps", 100)))
        sents = to_sents(remove_pad_eos(samples.cpu().numpy(), eos=self.vocab["<EOS>"]), self.vocab,
                         self.non_lang_syms)
        self.judge.train()
        return total / len(self.dev_loader), sents

    def test(self, state_dict=None, judge_state_dict=None):
        # `ctc_greedy_decode` (not a reference key; default false): decode with the CTC head alone, best path
        # (E2E.recognize_ctc) instead of the attention decoder - the head's own hypotheses.  It is a decoder
        # of its own: no beam, no judge, no prefix score.
        ctc_greedy = bool(self.config.get("ctc_greedy_decode", False))
        if ctc_greedy and (int(self.config.get("beam_size", 1) or 1) > 1 or float(self.config.get("lm_weight", 0.0) or 0.0) > 0
                           or float(self.config.get("ctc_decode_weight", 0.0) or 0.0) > 0):
            raise ValueError("ctc_greedy_decode decodes with the CTC head alone: it does not combine with beam_size > 1, "
                             "lm_weight > 0 or ctc_decode_weight > 0")
        # `rnnt_beam_decode` (not a reference key; default false): the transducer head's beam search, a decoder
        # of its own with a place for `ngram_lm`; the n-gram keys are its own then, and every other path below sees a
        # configuration without them.  Absent, nothing here differs from a configuration that never had the key.
        rnnt_beam = self.rnnt_beam_config(self.config, hasattr(self.model, "rnnt"))
        cfg = self.config
        if rnnt_beam:
            cfg = {k: v for k, v in self.config.items() if k not in ("ngram_lm", "ngram_weight", "ngram_bonus", "beam_size")}
        rnnt_greedy = self.rnnt_decode_config(cfg, hasattr(self.model, "rnnt"))
        two_pass = self.two_pass_config(cfg, hasattr(self.model, "ctc_lo"))
        ctc_beam, ngram_path, ngram_w, ngram_bonus = self.ngram_config(cfg, two_pass, hasattr(self.model, "ctc_lo"))
        if rnnt_beam and self.config.get("ngram_lm") is not None:
            ngram_path = self.config["ngram_lm"]
            ngram_w, ngram_bonus = (float(self.config.get(k, 0.0) or 0.0) for k in ("ngram_weight", "ngram_bonus"))
        ngram = None
        if ngram_path is not None:
            from ngram import NgramLM
            ngram = (NgramLM.from_arpa(ngram_path, {s: i for s, i in self.vocab.items() if s not in ("<s>", "</s>")},
                                       self.vocab["<BOS>"], self.vocab["<EOS>"], V=len(self.vocab)), ngram_w, ngram_bonus)
        wlm_path, lexicon_path, wlm_w, word_bonus, lexicon_only = self.word_lm_config(self.config, two_pass, ctc_beam)
        if wlm_path is not None:
            ngram = dict(word_lm=self.load_word_lm(wlm_path, lexicon_path), word_lm_weight=wlm_w, word_bonus=word_bonus,
                         lexicon_only=lexicon_only)
        # `context_bias` (not a reference key): a phrase list inside the CTC prefix beam search; absent, nothing
        # below differs
        ctx_sub = self.context_config(self.config, two_pass, ctc_beam and not rnnt_beam)
        if ctx_sub is not None:
            weight = ctx_sub.get("weight", 1.0)
            ngram = dict(self._lm_kwargs(ngram), context=self.load_context(ctx_sub), ctx_weight=float(1.0 if weight is None else weight))
        if rnnt_beam and self.config.get("rnnt_word_lm") is not None:
            # `rnnt_word_lm` (not a reference key): the lexicon and the word LM inside the transducer search
            rw = self.config["rnnt_word_lm"]
            ngram = dict(word_lm=self.load_word_lm(rw["arpa"], rw.get("lexicon")), word_lm_weight=float(rw.get("weight", 0.0) or 0.0),
                         word_bonus=float(rw.get("bonus", 0.0) or 0.0), lexicon_only=bool(rw.get("lexicon_only", False)))
        # `att_ngram_lm` / `att_word_lm` (not reference keys): the n-gram or the lexicon and word LM inside the
        # attention beam search; absent, nothing below differs
        att_kind, att_sub = self.att_lm_config(self.config)
        att_lm = None
        if att_kind == "ngram":
            from ngram import NgramLM
            att_lm = dict(ngram=NgramLM.from_arpa(att_sub["arpa"], {s: i for s, i in self.vocab.items() if s not in ("<s>", "</s>")},
                                                  self.vocab["<BOS>"], self.vocab["<EOS>"], V=len(self.vocab)),
                          ngram_weight=float(att_sub.get("weight", 0.0) or 0.0), ngram_bonus=float(att_sub.get("bonus", 0.0) or 0.0))
        elif att_kind == "word":
            att_lm = dict(word_lm=self.load_word_lm(att_sub["arpa"], att_sub.get("lexicon")),
                          word_lm_weight=float(att_sub.get("weight", 0.0) or 0.0), word_bonus=float(att_sub.get("bonus", 0.0) or 0.0),
                          lexicon_only=bool(att_sub.get("lexicon_only", False)))
        if state_dict:
            self.model.load_state_dict(state_dict)
        else:
            self.load_model(self.config["load_model_path"], self.config["load_optimizer"])
        # `lm_weight` (not a reference key, like beam_size): > 0 decodes with the judge's log-probabilities added to the
        # recogniser's, weighted (shallow fusion), also at beam_size 1; the judge is the one saved beside the recogniser
        lm_weight = float(self.config.get("lm_weight", 0.0) or 0.0)
        if lm_weight > 0:
            if judge_state_dict:
                self.judge.load_state_dict(judge_state_dict)
            else:
                self.load_judge(self.config["load_judge_path"], False)
            judge_was_training = self.judge.training
            self.judge.eval()
        # `ctc_decode_weight` (not a reference key): > 0 decodes with the CTC prefix score of the model's CTC head inside the
        # search (joint CTC-attention decoding), also at beam_size 1; it combines with lm_weight and is separate
        # from the training loss's `ctc_weight`, which must be > 0 for the head to exist
        ctc_w = float(self.config.get("ctc_decode_weight", 0.0) or 0.0)
        beam_size = int(self.config.get("beam_size", 1) or 1)    # not reference keys: beam_size, beam_length_penalty
        test_set = self.config["test_set"]
        loader = get_data_loader(self._dataset(test_set, None, sort=False), batch_size=1, shuffle=False,
                                 drop_last=False)
        self.model.eval()
        # with `cer_on_gpu` a beam search keeps all its K hypotheses per utterance: the best-of-K CER below; with `wer_on_gpu`
        # for the best-of-K WER (rank 0 of the list is the hypothesis the search returns without it)
        wer_dev = self._wer_device()
        nbest_cer = beam_size > 1 and self._cer_device() is not None
        nbest = nbest_cer or (beam_size > 1 and wer_dev is not None)
        preds, refs, beams = [], [], []
        for batch in self._feed(loader, sharded=False):
            xs, ilens, _ = batch
            if rnnt_beam and nbest:
                ranked = self._rnnt_beams(xs, ilens, beam_size, ngram, nbest=True)
                preds += [hyps[0] for hyps in ranked]
                beams += ranked
            elif rnnt_beam:
                preds += self._rnnt_beams(xs, ilens, beam_size, ngram)
            elif rnnt_greedy:
                preds += self._rnnt_greedy(xs, ilens)
            elif ctc_greedy:
                preds += self._ctc_best_path(xs, ilens)
            elif ctc_beam and nbest:
                ranked = self._ctc_beams(xs, ilens, beam_size, ngram, nbest=True)
                preds += [hyps[0] for hyps in ranked]
                beams += ranked
            elif ctc_beam:
                preds += self._ctc_beams(xs, ilens, beam_size, ngram)
            elif two_pass and nbest:
                ranked = self._two_pass(xs, ilens, beam_size, ctc_w, lm_weight, nbest=True, ngram=ngram)
                preds += [hyps[0] for hyps in ranked]
                beams += ranked
            elif two_pass:
                preds += self._two_pass(xs, ilens, beam_size, ctc_w, lm_weight, ngram=ngram)
            elif nbest:
                ranked = self._beam(xs, ilens, beam_size, lm_weight, nbest=True, ctc_decode_weight=ctc_w, table_lm=att_lm)
                preds += [hyps[0] for hyps in ranked]
                beams += ranked
            elif lm_weight > 0 or ctc_w > 0 or att_lm is not None:
                preds += self._beam(xs, ilens, beam_size, lm_weight, ctc_decode_weight=ctc_w, table_lm=att_lm)
            else:
                preds += self._beam(xs, ilens, beam_size) if beam_size > 1 else self._greedy(xs, ilens)
            refs += batch.ys_host
        self.model.train()
        if lm_weight > 0:
            self.judge.train(judge_was_training)
        self.last_test = dict(cer=None, best_of_k_cer=None, dist=None, ref_n=None)
        if nbest_cer:
            # every hypothesis of every utterance against the utterance's reference in one launch; a rank the search left
            # without a hypothesis is a row of <EOS>: an empty hypothesis.  The rank-0 rows give the CER itself.
            K = beam_size
            _, dist, ref_n = self._score_ids([h for hyps in beams for h in hyps], refs,
                                             ref_index=[b for b in range(len(beams)) for _ in range(K)])
            dist = [dist[b * K:(b + 1) * K] for b in range(len(beams))]
            ref_n = ref_n[::K]
            cer = float(sum(d[0] for d in dist)) / float(sum(ref_n))
            best_of_k = float(sum(min(d) for d in dist)) / float(sum(ref_n))
            self.last_test.update(best_of_k_cer=best_of_k, dist=dist, ref_n=ref_n)
            hyp_sents = to_sents(remove_pad_eos(preds, eos=self.vocab["<EOS>"]), self.vocab, self.non_lang_syms)
        else:
            cer, hyp_sents, _ = self.ind2sent(preds, refs)
        self.last_test["cer"] = cer
        words = ""
        if wer_dev is not None:
            # the same on words, one launch: the K hypotheses of every utterance (K = 1 without a beam) against its reference
            K = beam_size if nbest else 1
            _, wdist, wref_n = calculate_wer_ids([h for hyps in beams for h in hyps] if nbest else preds, refs, self.vocab,
                                                 self.non_lang_syms, self.vocab["<EOS>"], wer_dev,
                                                 ref_index=[b for b in range(len(refs)) for _ in range(K)])
            wdist = [wdist[b * K:(b + 1) * K] for b in range(len(refs))]
            wref_n = wref_n[::K]
            wer = float(sum(d[0] for d in wdist)) / float(sum(wref_n))
            self.last_test.update(wer=wer, word_dist=wdist, word_ref_n=wref_n)
            words = f", WER={wer:.4f}"
            if nbest:
                self.last_test["best_of_k_wer"] = float(sum(min(d) for d in wdist)) / float(sum(wref_n))
                words += f", best of {beam_size}: WER={self.last_test['best_of_k_wer']:.4f}"
        with open(f"{test_set}.txt", "w") as f:
            f.writelines(f"{p}\n" for p in hyp_sents)
        print(f"{test_set}: {len(hyp_sents)} utterances, CER={cer:.4f}"
              + (f", best of {beam_size} hypotheses: CER={self.last_test['best_of_k_cer']:.4f}" if nbest_cer else "") + words)
        return cer

    # ------------------------------------------------------------------ judge (LM) pre-training
    # Number of train steps whose host read may be outstanding when the next one is enqueued.  1 (default): the host looks
    # at step i's loss and abort latch while step i + 1 runs - no GPU idle time between steps.  0: the reference's order,
    # loss.item() inside every step (solver.py:379).  Config key `pipeline_steps` (not a reference key).
    PIPELINE_STEPS = 1
    PINNED_ROWS = 8                    # landing rows for the host records of outstanding steps: pipeline_steps <= PINNED_ROWS - 2

    def _step(self, make_local, opt, n_scalars):
        """Run one optimiser step on make_local() -> (local loss, [scalar tensors]); returns the scalars, summed over the
        ranks of a data-parallel run (= the single-process values), as StepScalars (plain floats from the synchronous
        data-parallel step, `pipeline_steps: 0`).

        One process: nothing in the step waits for the host.  zero_grad -> backward -> gradients into the flat buffer ->
        [loss scalars + abort latch -> pinned host memory, asynchronously] -> clip + Adam, whose kernel checks the abort latch
        ON THE DEVICE and does nothing when it is set (asr_adam_clip_f32: skip_if_nonzero).  The host reads a step's record
        while the NEXT step runs (the reference's per-step loss.item(), one step late).  The persistent XCD-local kernels
        poison their outputs with NaN and set the sticky latch when they abort (a workgroup placement other than one per CU,
        a bounded spin expiring: a shared or partitioned GPU); the latch stays set, so the update of the aborted step AND of
        every step enqueued behind it was skipped on the device - _recover switches this process to the per-step kernels
        and runs those steps again from the numpy stream (teacher-forcing draws) the first of them started with.  A
        non-finite loss without the latch is the model's own and is applied, as in the reference.

        Data parallel: the same, with the latch SUMMED OVER THE RANKS in the step's one all-reduce (last aux slot of the flat
        buffer) as the device-side predicate - every rank skips or none does - and the coordinated repeat one step late
        (parallel.DpPipeline).  Every rank resolves its StepScalars at the same points of the program (the loops
        below run the same code on all ranks): a recovery is a sequence of collectives."""
        dev0 = opt.buf.flat_g.device
        if hb.persistent_step_tick() and self.rank == 0:     # the end of a probation after an abort (hb.PERSIST_RETRY_STEPS)
            print("persistent kernels: trying them again after %d abort(s)" % hb.persistent_probation()[0])
        with hb.deterministic(self.deterministic), ops.step_arena(dev0):   # every zero-initialised accumulator of the step
            return self._step_inner(make_local, opt, n_scalars)           # comes out of one buffer, one fill

    def _step_inner(self, make_local, opt, n_scalars):
        depth = min(int(self.config.get("pipeline_steps", self.PIPELINE_STEPS)), self.PINNED_ROWS - 2)   # one landing row each
        if self.world > 1 or parallel.FORCE_DP:
            pipe = self._dp_pipeline(depth, opt.buf.flat_g.device)
            rec = pipe.step(make_local, opt, n_scalars)
            if depth <= 0:
                pipe.resolve(rec)                        # `pipeline_steps: 0`: the same path, read at once
            self._report_paths()
            return [StepScalar(rec, i) for i in range(n_scalars)]
        rec = dict(resolve=self._resolve_through, opt=opt, make_local=make_local, n=n_scalars, rng=np.random.get_state(),
                   values=None, event=None, slot=None)
        loss, scalars = make_local()
        opt.zero_grad()
        parallel.backward(loss)                          # (the seed of the backward pass is a cached tensor)
        opt.reduce()                                     # gradients -> flat buffer (no collective in one process)
        if not loss.is_cuda:                             # CPU tensors (tests of the host logic): nothing to pipeline
            opt.apply()
            rec["values"] = [float(v) for v in scalars[:n_scalars]]
            return [StepScalar(rec, i) for i in range(n_scalars)]
        dev = loss.device
        latch = hb.persist_abort_flag(dev)
        rec["slot"] = self._free_slot()
        stage = torch.stack([v.detach().reshape(()).float() for v in scalars[:n_scalars]] + [latch[0].float()])
        self._pinned[rec["slot"], :n_scalars + 1].copy_(stage, non_blocking=True)
        rec["event"] = torch.cuda.Event()
        rec["event"].record()
        opt.apply(skip_if=latch)                         # clip -> Adam; a no-op on the device if the latch is set
        self._pending.append(rec)
        while len(self._pending) > depth:
            self._resolve_through(self._pending[0])
        self._report_paths()
        return [StepScalar(rec, i) for i in range(n_scalars)]

    @staticmethod
    def settle_host_memory():
        """The corpora, vocabularies and loaders built so far live as long as the process: collect what is garbage now and move
        the rest out of the garbage collector's sight (gc.freeze).  A full collection that has to walk a corpus of a few
        thousand utterances (dicts of arrays and token lists) takes tens of milliseconds - and when it strikes in the middle
        of an epoch the host, one step ahead of the GPU, falls behind it (measured: a 60-batch epoch at cfg-2 ran 12.6 ms
        per step instead of 11.7, one 50 ms pause)."""
        import gc
        gc.collect()
        gc.freeze()

    def _free_slot(self):
        """A row of the pinned landing buffer that no outstanding step uses."""
        if self._pinned is None:
            self._pinned = torch.zeros(self.PINNED_ROWS, 8, dtype=torch.float32).pin_memory()
        busy = set(r["slot"] for r in self._pending)
        if self._dp_pipe is not None:
            row = self._pinned.stride(0) * self._pinned.element_size()
            busy |= set((r["host"].data_ptr() - self._pinned.data_ptr()) // row for r in self._dp_pipe.pending)
        return next(i for i in range(self._pinned.shape[0]) if i not in busy)

    def _dp_pipeline(self, depth, dev):
        """The data-parallel step (parallel.DpPipeline, the only one): the abort latch rides in the last aux slot of the step's
        ONE all-reduce, its sum predicates the update on the device - every rank skips or none does -, the reduced scalars
        land in pinned host memory behind an event; when a record shows the latch set EVERY rank leaves the persistent
        kernels (a rank that alone repeats a batch would be one collective the others do not take part in) and repeats what
        was skipped, from the numpy streams those steps started with."""
        if self._dp_pipe is None and dev.type != "cuda":           # (CPU tensors: tests of the host logic on gloo)
            self._dp_pipe = parallel.DpPipeline(max(1, depth), lambda: 0.0, lambda n: None)
        if self._dp_pipe is None:
            def stage(aux):
                host = self._pinned[self._free_slot(), :aux.numel()]
                host.copy_(aux, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                return host, event.synchronize

            def latch():
                return hb.persist_abort_flag(torch.device("cuda", torch.cuda.current_device()))[0].float()

            def leave_persistent(n_ranks):
                dev = torch.device("cuda", torch.cuda.current_device())
                torch.cuda.synchronize()
                print("rank %d: persistent kernels aborted on %d rank(s) (this rank: %s, code %d): every rank repeats the "
                      "skipped step(s) on the per-step kernels" % (self.rank, n_ranks, hb.persist_aborted(dev),
                                                                   hb.persist_abort_code(dev)))
                hb.disable_persistent(dev)              # also clears this rank's latch
            self._free_slot()                           # allocates the pinned buffer
            self._dp_pipe = parallel.DpPipeline(depth, latch, leave_persistent, stage)
        self._dp_pipe.depth = max(1, int(depth))
        return self._dp_pipe

    def _report_paths(self):
        if not self._paths_reported:
            # which kernels the sequence operators of the first step ran on (hb.LAUNCHES: *_persist = the persistent
            # XCD-local kernels, *_step = the per-step kernels, 3x slower: unsupported width, shared or partitioned GPU)
            self._paths_reported = True
            if self.rank == 0:
                print("sequence-operator paths of the first step: %s (persistent kernels %s)"
                      % (dict(sorted(hb.LAUNCHES.items())), "on" if hb.USE_PERSIST else "off"))

    def _resolve_through(self, rec):
        """Read the host records of every outstanding step up to and including `rec` (oldest first)."""
        while self._pending and rec["values"] is None:
            first = self._pending[0]
            first["event"].synchronize()
            vals = self._pinned[first["slot"], :first["n"] + 1].tolist()
            if vals[-1] != 0.0:
                self._recover()
            else:
                first["values"] = vals[:first["n"]]
                first["make_local"] = first["opt"] = None   # a StepScalar kept in a log must not keep the batch alive
                self._pending.pop(0)

    def _lagged(self, log):
        """-> (push, done): push(item) reports the PREVIOUS item through log(item) - its step's host record has landed by
        then, so printing its loss does not make the host wait for the step that was just enqueued - and done() reports
        the last one (the reference prints every step's loss inside the step, solver.py:379-381)."""
        held = []

        def push(item):
            if held:
                log(held.pop())
            held.append(item)

        def done():
            if held:
                log(held.pop())
        return push, done

    def flush(self):
        """Wait for the host records of all outstanding train steps (before validation, checkpoints, the end of a loop)."""
        while self._pending:
            self._resolve_through(self._pending[-1])
        if self._dp_pipe is not None:
            self._dp_pipe.flush()

    def _recover(self):
        """The oldest outstanding step found the abort latch set: neither its update nor that of any step enqueued behind it
        was applied (the latch is sticky and the Adam kernel checks it on the device).  Leave the persistent kernels (until
        the probation of hip_backend.persistent_step_tick ends), take the optimisers' step counts back and run those steps
        again, in order, each from the numpy stream it started with and in an arena scope of its own (this may run at the end
        of the step that found the abort, inside ITS scope: that step is fully enqueued by then and hands back scalars only,
        so its slices may be zeroed - ops._Arena, LIFETIME)."""
        torch.cuda.synchronize()
        redo, self._pending = self._pending, []
        dev = redo[0]["opt"].buf.flat_g.device
        print("persistent kernels aborted (code %d): continuing on the per-step kernels, repeating %d step(s)"
              % (hb.persist_abort_code(dev), len(redo)))
        hb.disable_persistent(dev)                       # also clears the latch
        for rec in redo:
            rec["opt"].unapply()
        resume = np.random.get_state()                   # where the stream stands now: behind every draw made so far
        for rec in redo:
            # each step again from the stream state IT started with: draws made between the steps (none in the loops of
            # this file - the input noise has a stream of its own, feed.DeviceFeed - but a caller may make some) are not
            # part of a step and must not shift the teacher-forcing draws of the repeats
            np.random.set_state(rec["rng"])
            with hb.deterministic(self.deterministic), ops.step_arena(dev):
                loss, scalars = rec["make_local"]()
                rec["opt"].zero_grad()
                loss.backward()
                both = torch.stack([v.detach().reshape(()).float() for v in scalars[:rec["n"]]] +
                                   [hb.persist_abort_flag(dev)[0].float()]).tolist()
                if both[-1] != 0.0:
                    raise RuntimeError("the abort latch is set (code %d) after a step on the per-step kernels"
                                       % hb.persist_abort_code(dev))
                rec["opt"].step()
            rec["values"] = both[:rec["n"]]
            rec["make_local"] = rec["opt"] = None
        np.random.set_state(resume)                      # a step draws the same number of values whatever its outputs were

    def judge_train_one_iteration(self, unlab_ys):
        """solver.py:288-301.  `unlab_ys` is the global text batch - every rank of a data-parallel run takes its strided
        shard and normalises by the global sum of (len + 5) (parallel.judge_local_loss; the identity for one process) - or
        this rank's parallel.LocalShard of it (the loops below: only the shard was uploaded)."""
        def make_local():
            loss, avg_prob = parallel.judge_local_loss(
                lambda ys: self.judge(ys=ys, discrete_input=True),
                lambda v, ys: self.judge.mask_and_cal_sum(v, ys=ys, mask=None), unlab_ys, self.rank, self.world)
            return loss, [loss, avg_prob]
        value, avg_prob = self._step(make_local, self.dis_opt, 2)
        return {"loss": value, "avg_prob": avg_prob}

    def judge_pretrain(self):
        cfg = self.config
        steps_per_epoch = len(self.train_unlab_y_loader)
        best = 100
        base_lr = cfg["d_learning_rate"]
        path = os.path.join(cfg["model_dir"], cfg["model_name"])
        print("--------Judge pretraining--------")
        for epoch in range(cfg["judge_epochs"]):
            # MultiStepLR(milestones=[dis_change_learning_rate_epoch], gamma) stepped at epoch start (solver.py:308-315)
            adjust_learning_rate(self.dis_opt, base_lr * (cfg["lr_gamma"] if epoch + 1 >= cfg[
                "dis_change_learning_rate_epoch"] else 1.0))
            total = [0.0]

            def log(item):
                it, meta = item
                total[0] += float(meta["loss"])
                print(f"epoch: {epoch}, [{it + 1}/{steps_per_epoch}], loss: {meta['loss']:.3f}, "
                      f"prob: {meta['avg_prob']:.3f}", end="\r")
                for key, val in meta.items():
                    self.logger.scalar_summary(f"{cfg['tag']}/judge_pretrain/{key}", float(val),
                                               epoch * steps_per_epoch + it + 1)
            push, done = self._lagged(log)
            for it, batch in enumerate(self._feed(self.train_unlab_y_loader, kind="text")):
                push((it, self.judge_train_one_iteration(batch.xs if self.world > 1 else batch.ys)))
            done()
            running = total[0]
            val_loss, samples = self.lm_validation()
            print(f"epoch: {epoch}, train_loss={running / steps_per_epoch:.3f}, valid_loss={val_loss:.3f}")
            for i, s in enumerate(samples):
                print(f"hyp-{i + 1}: {s}")
            self.logger.scalar_summary(f"{cfg['tag']}/judge_pretrain/val_loss", val_loss, epoch)
            self.logger.scalar_summary(f"{cfg['tag']}/judge_pretrain/avg_train_loss", running / steps_per_epoch, epoch)
            if val_loss < best:
                best = val_loss
                self.save_judge(path)
                print(f"save #{epoch} LM, val_loss={val_loss:.3f}")
            self.save_judge(f"{path}-{epoch:03d}")

    # ------------------------------------------------------------------ supervised training
    def _sharded_forward(self, xs, ilens, ys, tf_rate):
        """Model forward on this rank's strided shard of the (global) batch, padded to the global extents;
        returns the local loss whose all-reduced gradient equals the single-process one; None for a rank
        whose shard is empty (fewer utterances than ranks in the last batch of an epoch).  One process: the whole
        batch and -mean(log_probs) (solver.py:375-378)."""
        cfg = self.config
        return parallel.sup_local_loss(self.model, xs, ilens, ys, tf_rate, self.rank, self.world,
                                       cfg["enc_n_layers"], cfg["subsample"])

    def sup_train_one_iteration(self, xs, ilens, ys, tf_rate):
        """The body of the supervised loop (solver.py:375-385) for one batch already on the device - the global batch, or this
        rank's parallel.LocalShard of it as `xs` (what the epoch loop's feed uploads under data parallelism): forward on this
        rank's shard, loss = -mean(log_probs), zero_grad, backward, (all-reduce,) loss + abort latch read on the host - the
        reference's loss.item() - then clip + Adam.  bench.py times exactly this method."""
        def make_local():
            loss = self._sharded_forward(xs, ilens, ys, tf_rate)
            return loss, [loss]
        value, = self._step(make_local, self.gen_opt, 1)         # (all-reduce ->) clip -> Adam; local losses sum to the mean
        return value

    def sup_train_one_epoch(self, epoch, tf_rate):
        cfg = self.config
        steps_per_epoch = len(self.train_lab_loader)
        running = [0.0]

        def log(item):
            it, value = item
            running[0] += float(value)
            if self.rank == 0:
                print(f"epoch: {epoch}, [{it + 1}/{steps_per_epoch}], loss: {value:.3f}", end="\r")
            self.logger.scalar_summary(tag=f"{cfg['tag']}/train_loss", value=float(value),
                                       step=epoch * steps_per_epoch + it + 1)
        push, done = self._lagged(log)
        # input noise (solver.py:370-373) is added by the feed, on the host, before the upload
        noise = float(cfg["gaussian_std"]) if cfg["add_gaussian"] and epoch >= cfg["gaussian_epoch"] else 0.0
        for it, (xs, ilens, ys) in enumerate(self._feed(self.train_lab_loader, noise_std=noise, train=True)):
            push((it, self.sup_train_one_iteration(xs, ilens, ys, tf_rate)))
        done()
        return running[0] / steps_per_epoch

    def sup_pretrain(self):
        cfg = self.config
        self.model.train()
        best_cer, best_model = 200, None
        hi, lo, span = cfg["init_tf_rate"], cfg["tf_rate_lowerbound"], cfg["tf_decay_epochs"]
        path = os.path.join(cfg["model_dir"], cfg["model_name"])
        print("------supervised pretraining-------")
        for epoch in range(cfg["epochs"]):
            tf_rate = hi - (hi - lo) * (epoch / span) if epoch <= span else lo
            train_loss = self.sup_train_one_epoch(epoch, tf_rate)
            val_loss, cer, hyps, refs = self.validation()
            print(f"Epoch: {epoch}, tf_rate={tf_rate:.3f}, train_loss={train_loss:.4f}, "
                  f"valid_loss={val_loss:.4f}, CER={cer:.4f}")
            tag = cfg["tag"]
            self.logger.scalar_summary(f"{tag}/supervised/cer", cer, epoch)
            self.logger.scalar_summary(f"{tag}/supervised/val_loss", val_loss, epoch)
            self.logger.scalar_summary(f"{tag}/supervised/avg_train_loss", train_loss, epoch)
            for i, (p, gt) in enumerate(list(zip(hyps, refs))[:5]):
                self.logger.text_summary(f"{tag}/supervised/prediction-{i}", p, epoch)
                self.logger.text_summary(f"{tag}/supervised/ground_truth-{i}", gt, epoch)
                print(f"hyp-{i + 1}: {p}\nref-{i + 1}: {gt}")
            if cer < best_cer:
                best_cer = cer
                self.save_model(path)
                best_model = self.model.state_dict()
                print(f"Save #{epoch} model, val_loss={val_loss:.3f}, CER={cer:.3f}")
            self.save_model(f"{path}-{epoch:03d}")
        return best_model, best_cer

    # ------------------------------------------------------------------ minimum error rate training
    @staticmethod
    def mwer_config(config, world=1):
        """The MWER keys of the configuration -> (K, ce_weight, epochs), or None when `mwer_beam` is absent (off).  ValueError
        for a beam outside 2..16, a negative weight, no epochs, or more than one process."""
        if config.get("mwer_beam") is None:
            return None
        K = int(config["mwer_beam"])
        if not 2 <= K <= hb.BEAM_KMAX:
            raise ValueError("mwer_beam %d outside 2..%d" % (K, hb.BEAM_KMAX))
        ce_weight, epochs = float(config.get("mwer_ce_weight", 0.01)), int(config.get("mwer_epochs", 1))
        if ce_weight < 0 or epochs < 1:
            raise ValueError("mwer_ce_weight %g must be >= 0 and mwer_epochs %d >= 1" % (ce_weight, epochs))
        if int(world) > 1:
            raise ValueError("MWER training runs in one process: data-parallel MWER (world size %d) is not supported" % world)
        return K, ce_weight, epochs

    @staticmethod
    def mwer_unit_config(config, vocab):
        """`mwer_unit` (not a reference key): `token` (default; the risk counts token errors) or `word` (word errors: the
        hypotheses and references are split at <space>) -> None for `token`, the id of <space> for `word`.
        ValueError for any other value, and for `word` with a vocabulary that has no <space>."""
        unit = config.get("mwer_unit", "token")
        if unit not in ("token", "word"):
            raise ValueError("mwer_unit %r is neither 'token' nor 'word'" % (unit,))
        if unit == "token":
            return None
        if "<space>" not in vocab:
            raise ValueError("mwer_unit 'word' needs <space> in the vocabulary: words are what lies between two of them")
        return int(vocab["<space>"])

    def mwer_train_one_iteration(self, xs, ilens, ys, hyps=None):
        """One minimum-error-rate step on a batch already on the device: E2E.mwer_forward (encoder, n-best
        search under no_grad - or the given `hyps` -, edit distances, scoring pass, risk loss, + mwer_ce_weight times the
        supervised loss), backward, the fused clip + Adam.  -> (loss, mean risk) as StepScalars; nothing is read on the host
        inside the step."""
        mw = self.mwer_config(self.config, self.world)
        if mw is None:
            raise ValueError("mwer_train_one_iteration needs `mwer_beam` in the configuration")
        K, ce_weight, _ = mw
        xs, ilens, ys, _ = parallel.shard_batch(xs, ilens, ys, 0, 1)      # (a LocalShard of a one-process feed passes through)

        def make_local():
            loss = self.model.mwer_forward(xs, ilens, ys, K, ce_weight=ce_weight,
                                           max_dec_timesteps=self.config["max_dec_timesteps"], hyps=hyps,
                                           unit="token" if self.mwer_space is None else "word")
            return loss, [loss, self.model.last_mwer["mwer"]]
        loss, risk = self._step(make_local, self.gen_opt, 2)
        return loss, risk

    def mwer_train(self):
        """`mwer_epochs` epochs of MWER steps over the labeled set, the dev CER after each as sup_pretrain reports it;
        checkpoints by sup_pretrain's rule (the best CER under model_name, every epoch under model_name-mwer-NNN)."""
        cfg = self.config
        mw = self.mwer_config(cfg, self.world)
        if mw is None:
            raise ValueError("mwer_train needs `mwer_beam` in the configuration")
        K, ce_weight, epochs = mw
        self.model.train()
        best_cer, best_model = 200, None
        path = os.path.join(cfg["model_dir"], cfg["model_name"])
        steps_per_epoch = len(self.train_lab_loader)
        print("------minimum error rate training (%d-best, ce weight %g)-------" % (K, ce_weight))
        for epoch in range(epochs):
            running = [0.0, 0.0]

            def log(item):
                it, (loss, risk) = item
                running[0] += float(loss)
                running[1] += float(risk)
                if self.rank == 0:
                    print(f"epoch: {epoch}, [{it + 1}/{steps_per_epoch}], loss: {loss:.3f}, risk: {risk:.3f}", end="\r")
                self.logger.scalar_summary(tag=f"{cfg['tag']}/mwer/train_loss", value=float(loss),
                                           step=epoch * steps_per_epoch + it + 1)
            push, done = self._lagged(log)
            for it, (xs, ilens, ys) in enumerate(self._feed(self.train_lab_loader, train=True)):
                push((it, self.mwer_train_one_iteration(xs, ilens, ys)))
            done()
            train_loss, train_risk = running[0] / steps_per_epoch, running[1] / steps_per_epoch
            val_loss, cer, hyps, refs = self.validation()
            print(f"Epoch: {epoch}, train_loss={train_loss:.4f}, train_risk={train_risk:.4f}, "
                  f"valid_loss={val_loss:.4f}, CER={cer:.4f}")
            tag = cfg["tag"]
            self.logger.scalar_summary(f"{tag}/mwer/cer", cer, epoch)
            self.logger.scalar_summary(f"{tag}/mwer/val_loss", val_loss, epoch)
            self.logger.scalar_summary(f"{tag}/mwer/avg_train_loss", train_loss, epoch)
            self.logger.scalar_summary(f"{tag}/mwer/avg_train_risk", train_risk, epoch)
            if cer < best_cer:
                best_cer = cer
                self.save_model(path)
                best_model = self.model.state_dict()
                print(f"Save #{epoch} model, val_loss={val_loss:.3f}, CER={cer:.3f}")
            self.save_model(f"{path}-mwer-{epoch:03d}")
        return best_model, best_cer

    # ------------------------------------------------------------------ n-best pseudo-labelling with the graph CTC loss
    PSEUDO_KEYS = ("pseudo_beam", "pseudo_temperature", "pseudo_weight", "pseudo_epochs")

    @staticmethod
    def pseudo_config(config, world=1, has_ctc_head=True):
        """The pseudo-labelling keys (not reference keys; all absent by default = off) -> None when `pseudo_beam`
        is absent, else (K, temperature, weight, epochs, ngram): `pseudo_beam` K in 2..16 hypotheses of the CTC prefix beam
        search per unlabeled utterance, weighed by the softmax of `pseudo_temperature` (default 1) times their scores;
        `pseudo_weight` (default 1) times the mean graph CTC loss is the step's loss; `pseudo_epochs` (default 1) passes of
        Solver.pseudo_train over the unlabeled speech.  `ngram_lm` (with `ngram_weight`, `ngram_bonus`) sits inside the search
        when it is configured: ngram is (path, weight, bonus) or None.  ValueError: a beam outside 2..16, a temperature or
        weight that is negative or not finite, no epochs, another pseudo key or an n-gram weight without what it belongs to,
        `word_lm` (the search of the pseudo-labels has no place for it), a model without the CTC head, more than one
        process.  `pseudo_graphs_on_gpu` is read by its own accessor (pseudo_graphs_on_gpu); without pseudo_beam it raises
        here like the other pseudo keys."""
        if config.get("pseudo_beam") is None:
            for key in Solver.PSEUDO_KEYS[1:] + ("pseudo_graphs_on_gpu",):
                if config.get(key) is not None:
                    raise ValueError("%s is set without pseudo_beam, the width of the n-best search it belongs to" % key)
            return None
        K = int(config["pseudo_beam"])
        if not 2 <= K <= hb.BEAM_KMAX:
            raise ValueError("pseudo_beam %d outside 2..%d" % (K, hb.BEAM_KMAX))
        temp = config.get("pseudo_temperature")
        weight = config.get("pseudo_weight")
        epochs = config.get("pseudo_epochs")
        temp, weight, epochs = (1.0 if temp is None else float(temp), 1.0 if weight is None else float(weight),
                                1 if epochs is None else int(epochs))
        if not (0 <= temp < float("inf")) or not (0 <= weight < float("inf")) or epochs < 1:
            raise ValueError("pseudo_temperature %g and pseudo_weight %g must be finite and >= 0, pseudo_epochs %d >= 1"
                             % (temp, weight, epochs))
        ngram = None
        if config.get("ngram_lm") is None:
            for key in ("ngram_weight", "ngram_bonus"):
                if key in config:
                    raise ValueError("%s is set without ngram_lm, the ARPA file it weighs" % key)
        else:
            ngram = (config["ngram_lm"], float(config.get("ngram_weight", 0.0) or 0.0), float(config.get("ngram_bonus", 0.0) or 0.0))
        if config.get("word_lm") is not None:
            raise ValueError("pseudo_beam searches with the CTC head and, at most, ngram_lm: word_lm has no place in it")
        if not has_ctc_head:
            raise ValueError("pseudo_beam needs the CTC head: build the model with ctc_weight > 0")
        if int(world) > 1:
            raise ValueError("pseudo-label training runs in one process: data-parallel pseudo-labelling (world size %d) is "
                             "not supported" % world)
        return K, temp, weight, epochs, ngram

    @staticmethod
    def pseudo_graphs_on_gpu(config):
        """The key `pseudo_graphs_on_gpu` (not a reference key; absent or false = off) -> bool: with it the
        pseudo-label step builds its graphs on the device (ops.gtc_nbest_graphs) and reads nothing back.  It belongs to
        `pseudo_beam`: ValueError without it, as for the other pseudo keys (pseudo_config raises the same)."""
        on = config.get("pseudo_graphs_on_gpu")
        if on is not None and config.get("pseudo_beam") is None:
            raise ValueError("pseudo_graphs_on_gpu is set without pseudo_beam, the width of the n-best search it belongs to")
        return bool(on)

    def _pseudo_ngram(self, spec):
        """The NgramLM of the pseudo-label search as _ctc_beams takes it, loaded once."""
        if spec is None:
            return None
        if getattr(self, "_pseudo_lm", None) is None or self._pseudo_lm[0] != spec[0]:
            from ngram import NgramLM
            lm = NgramLM.from_arpa(spec[0], {s: i for s, i in self.vocab.items() if s not in ("<s>", "</s>")},
                                   self.vocab["<BOS>"], self.vocab["<EOS>"], V=len(self.vocab))
            self._pseudo_lm = (spec[0], lm)
        return self._pseudo_lm[1], spec[1], spec[2]

    def pseudo_graphs(self, xs, ilens, K, temperature, ngram=None):
        """The n-best pseudo-labels of one unlabeled batch as label graphs: under no_grad and in eval mode the CTC prefix beam
        search (E2E.recognize_ctc_beams, nbest) with beam width K - its ONE device-to-host read of (hyp, hyp_len, score) is the
        only one of the step -, gtc.nbest_weights over every row's list, gtc.Graph.from_nbest per row.  -> (gtc.GraphBatch,
        the id lists, the log weights) ; the model is left in the mode it came in."""
        import gtc
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                ids, scores = self.model.recognize_ctc_beams(xs, ilens, K, nbest=True, **self._lm_kwargs(ngram))
        finally:
            self.model.train(was_training)
        B = len(ids)
        score = np.full((B, K), -np.inf)
        hyp_len = np.full((B, K), -1, dtype=np.int64)
        for b in range(B):
            n = len(ids[b])
            score[b, :n] = scores[b]
            hyp_len[b, :n] = [len(h) for h in ids[b]]
        logw = gtc.nbest_weights(score, hyp_len, temperature)
        V = self.model.ctc_lo.out_features
        graphs = []
        for b in range(B):
            live = [k for k in range(len(ids[b])) if logw[b, k] > -np.inf]
            if live:
                graphs.append(gtc.Graph.from_nbest([ids[b][k] for k in live], [logw[b, k] for k in live], V))
            else:                                       # (a search that kept nothing: the empty hypothesis)
                graphs.append(gtc.Graph.from_nbest([[]], [0.0], V))
        return gtc.GraphBatch(graphs, range(B)), ids, logw

    def pseudo_train_one_iteration(self, unlab_xs, unlab_ilens, lab=None, tf_rate=1.0):
        """One pseudo-label step on an unlabeled batch already on the device: the n-best search and its graphs
        (pseudo_graphs), then the encoder in training mode, loss = pseudo_weight * mean E2E.gtc_nll - plus, with lab =
        (xs, ilens, ys), the supervised loss of that labeled batch - through the step every other loop takes (_step).
        -> (loss, mean graph CTC loss) as StepScalars; self.last_pseudo keeps the graphs, id lists and log weights of the
        call.  That path reads the n-best list to the host and compiles the graphs there.  With `pseudo_graphs_on_gpu` (DESIGN
        4.37) the list stays on the device: E2E.ctc_beams_on_device, ops.gtc_nbest_graphs, then the same step on that table -
        no host read between entry and _step; self.last_pseudo then keeps device tensors: hyp, hyp_len, score, log_weights,
        dropped, and the table under graphs."""
        ps = self.pseudo_config(self.config, self.world, hasattr(self.model, "ctc_lo"))
        if ps is None:
            raise ValueError("pseudo_train_one_iteration needs `pseudo_beam` in the configuration")
        K, temperature, weight, _, ngram_spec = ps
        xs, ilens, _, _ = parallel.shard_batch(unlab_xs, unlab_ilens, None, 0, 1)    # (a one-process LocalShard passes through)
        if self.pseudo_graphs_on_gpu(self.config):
            was_training = self.model.training
            self.model.eval()
            try:
                with torch.no_grad():
                    hyp, hyp_len, score = self.model.ctc_beams_on_device(xs, ilens, K,
                                                                         **self._lm_kwargs(self._pseudo_ngram(ngram_spec)))
                    batch = ops.gtc_nbest_graphs(hyp, hyp_len, score, self.model.ctc_lo.out_features, temperature)
            finally:
                self.model.train(was_training)
            self.last_pseudo = dict(graphs=batch, hyp=hyp, hyp_len=hyp_len, score=score, log_weights=batch.log_weights,
                                    dropped=batch.dropped)
        else:
            batch, ids, logw = self.pseudo_graphs(xs, ilens, K, temperature, self._pseudo_ngram(ngram_spec))
            self.last_pseudo = dict(graphs=batch, ids=ids, log_weights=logw)

        def make_local():
            enc_h, _ = self.model.encoder(xs, ilens)
            gtc_mean = self.model.gtc_nll(enc_h, batch).sum() * (1.0 / len(ilens))
            loss = weight * gtc_mean
            if lab is not None:
                loss = loss + self._sharded_forward(lab[0], lab[1], lab[2], tf_rate)
            return loss, [loss, gtc_mean]
        loss, gtc_mean = self._step(make_local, self.gen_opt, 2)
        return loss, gtc_mean

    def pseudo_train(self):
        """`pseudo_epochs` passes of pseudo-label steps over the unlabeled speech (main.py --pseudo_train), the dev CER after
        each as sup_pretrain reports it; checkpoints by sup_pretrain's rule (the best CER under model_name, every epoch under
        model_name-pseudo-NNN)."""
        cfg = self.config
        ps = self.pseudo_config(cfg, self.world, hasattr(self.model, "ctc_lo"))
        if ps is None:
            raise ValueError("pseudo_train needs `pseudo_beam` in the configuration")
        K, temperature, weight, epochs, _ = ps
        self.model.train()
        best_cer, best_model = 200, None
        path = os.path.join(cfg["model_dir"], cfg["model_name"])
        steps_per_epoch = len(self.train_unlab_x_loader)
        print("------pseudo-label training (%d-best, temperature %g, weight %g)-------" % (K, temperature, weight))
        for epoch in range(epochs):
            running = [0.0]

            def log(item):
                it, (loss, gtc_mean) = item
                running[0] += float(loss)
                if self.rank == 0:
                    print(f"epoch: {epoch}, [{it + 1}/{steps_per_epoch}], loss: {loss:.3f}, gtc: {gtc_mean:.3f}", end="\r")
                self.logger.scalar_summary(tag=f"{cfg['tag']}/pseudo/train_loss", value=float(loss),
                                           step=epoch * steps_per_epoch + it + 1)
            push, done = self._lagged(log)
            for it, (xs, ilens) in enumerate(self._feed(self.train_unlab_x_loader, kind="speech", train=True)):
                push((it, self.pseudo_train_one_iteration(xs, ilens)))
            done()
            val_loss, cer, hyps, refs = self.validation()
            print(f"Epoch: {epoch}, train_loss={running[0] / steps_per_epoch:.4f}, valid_loss={val_loss:.4f}, CER={cer:.4f}")
            self.logger.scalar_summary(f"{cfg['tag']}/pseudo/cer", cer, epoch)
            self.logger.scalar_summary(f"{cfg['tag']}/pseudo/val_loss", val_loss, epoch)
            if cer < best_cer:
                best_cer = cer
                self.save_model(path)
                best_model = self.model.state_dict()
                print(f"Save #{epoch} model, val_loss={val_loss:.3f}, CER={cer:.3f}")
            self.save_model(f"{path}-pseudo-{epoch:03d}")
        return best_model, best_cer

    # ------------------------------------------------------------------ semi-supervised training
    def gen_train_one_iteration(self, lab_xs, lab_ilens, lab_ys, unlab_xs, unlab_ilens):
        """The LM-judge auxiliary loss (solver.py:460-495): greedy smooth-embedding decode of unlabeled
        speech WITH grad, judge probabilities of the hypothesis, unsup = -sum(p_LM * log p_model * mask)/sum(mask);
        loss = sup + unsup_weight * unsup; only the generator is stepped.
        lab_* / unlab_* are the GLOBAL batches (the loaders draw batch_size * world utterances) or this rank's
        parallel.LocalShards of them as lab_xs / unlab_xs: every rank works on its strided shards at the global padded extents and normalises the auxiliary loss by the global hypothesis-token
        count (parallel.ssl_local_loss: one 4-byte all-reduce next to the gradient all-reduce; nothing in one process)."""
        cfg = self.config

        def judge_probs(hyp):
            # The judge scores an integer hypothesis, so no gradient reaches the model through it, and gen_opt does not
            # hold its parameters (solver.py:484-488 builds that graph and never uses it): the forward alone gives the
            # same losses and model gradients.
            with torch.no_grad():
                return self.judge(ys=hyp, discrete_input=False)[1]

        def make_local():
            loss, (unsup, sup) = parallel.ssl_local_loss(
                self.model, judge_probs, (lab_xs, lab_ilens, lab_ys), (unlab_xs, unlab_ilens), self.rank, self.world,
                eos=self.vocab["<EOS>"], unsup_weight=cfg["unsup_weight"], proportion=self.proportion,
                smooth=cfg["smooth_embedding"], scaling=cfg["softmax_scaling"], n_layers=cfg["enc_n_layers"],
                subsample=cfg["subsample"])
            return loss, [unsup, sup, loss]
        unsup, sup, value = self._step(make_local, self.gen_opt, 3)
        return {"unsup_loss": unsup, "sup_loss": sup, "loss": value}

    def ssl_train_one_iteration(self, iteration):
        lab_xs, lab_ilens, lab_ys = next(self.lab_iter)
        unlab_xs, unlab_ilens = next(self.unlab_x_iter)
        return self.gen_train_one_iteration(lab_xs, lab_ilens, lab_ys, unlab_xs, unlab_ilens)

    def ssl_train(self):
        cfg = self.config
        print("--------SSL training--------")
        adjust_learning_rate(self.gen_opt, cfg["g_learning_rate"])
        best_cer, best_model = 2, None
        total = cfg["ssl_iterations"]
        path = os.path.join(cfg["model_dir"], cfg["model_name"])
        if not hasattr(self, "lab_iter"):
            self.get_infinite_iter()
        def log(item):
            it, meta = item
            print(f"[{it + 1}/{total}], sup_loss: {meta['sup_loss']:.3f}, unsup_loss: {meta['unsup_loss']:.3f}, "
                  f"loss: {meta['loss']:.3f}", end="\r")
            for key, val in meta.items():
                self.logger.scalar_summary(f"{cfg['tag']}/ssl_generator/{key}", float(val), it + 1)
        push, done = self._lagged(log)
        for step in range(total):
            push((step, self.ssl_train_one_iteration(iteration=step)))
            if (step + 1) % cfg["summary_steps"] == 0 or step + 1 == total:
                done()
                val_loss, cer, hyps, refs = self.validation()
                print(f"Iter: [{step + 1}/{total}], valid_loss={val_loss:.4f}, CER={cer:.4f}")
                self.logger.scalar_summary(f"{cfg['tag']}/ssl/cer", cer, step + 1)
                self.logger.scalar_summary(f"{cfg['tag']}/ssl/val_loss", val_loss, step + 1)
                for i, (p, gt) in enumerate(list(zip(hyps, refs))[:5]):
                    print(f"hyp-{i + 1}: {p}\nref-{i + 1}: {gt}")
                if cer < best_cer:
                    best_cer = cer
                    self.save_model(path)
                    self.save_judge(path)
                    best_model = self.model.state_dict()
                    print(f"Save #{step} model, val_loss={val_loss:.3f}, CER={cer:.3f}")
        return best_model, best_cer
