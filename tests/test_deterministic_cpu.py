"""Deterministic mode, the parts that need no GPU: the K split of asr_gemm_det_f32 as asr_gemm_det_ws_bytes reports
it, the Solver's refusal of `deterministic` with `dp_overlap`, the side stream."""
import os
import pickle

import pytest

import __graft_entry__ as entry

ASR_E_ARG, ASR_E_SHAPE = -1, -2


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    return hip_backend


def _rule(M, N, K):
    """include/asr_hip.h, asr_gemm_det_f32: the K ranges asked for when the caller names none."""
    tiles = -(-M // 128) * -(-N // 128)
    if K < 1024 or tiles >= 256:
        return 1
    return max(1, min(16, 256 // tiles, K // 512))


def _ranges(K, want):
    """... and the ranges that exist: (S, length of a range)."""
    want = max(1, min(want, K))
    kp = -(-K // want)
    if kp >= 32:
        kp = -(-kp // 32) * 32
    return -(-K // kp), kp


@pytest.mark.parametrize("M,N,K", [(4096, 80, 20000), (2048, 512, 5248), (512, 2048, 1024), (80, 80, 1023), (3200, 512, 512),
                                   (12800, 512, 4096), (4096, 8192, 4096), (1, 1, 1), (130, 17, 2051), (640, 36, 3200)])
def test_ws_bytes_follow_the_documented_rule(hb, M, N, K):
    S, kp = _ranges(K, _rule(M, N, K))
    for ta, tb in ((False, False), (True, False), (False, True), (True, True)):
        got = [hb.gemm_det_split(M, N, K, trans_a=ta, trans_b=tb) for _ in range(3)]
        assert got[0] == got[1] == got[2], "the answer is a function of the arguments"
        assert got[0]["rc"] == 0 and got[0]["split"] == S, (got[0], S)
        assert got[0]["bytes"] == (0 if S == 1 else S * M * N * 4), got[0]
        if S > 1:
            assert got[0]["k_range"] == kp and (S - 1) * kp < K <= S * kp


def test_the_rule_splits_the_long_weight_gradient_products_and_nothing_short(hb):
    assert hb.gemm_det_split(4096, 80, 20000, trans_a=True)["split"] == 8          # layer-0 dW_ih: 32 tiles
    assert hb.gemm_det_split(3200, 512, 512, trans_b=True)["bytes"] == 0          # a forward projection
    assert hb.gemm_det_split(4096, 8192, 4096)["bytes"] == 0                      # tiles fill the chip


@pytest.mark.parametrize("split", [2, 3, 7])
@pytest.mark.parametrize("K", [1, 5, 63, 1000, 2051])
def test_an_explicit_split_is_honoured_up_to_k(hb, split, K):
    S, kp = _ranges(K, split)
    got = hb.gemm_det_split(17, 130, K, split=split)
    assert got["rc"] == 0 and got["split"] == S and got["bytes"] == (0 if S == 1 else S * 17 * 130 * 4), got
    assert S <= split and S <= K


def test_refusals_mirror_asr_gemm_f32(hb):
    for kw in (dict(M=0, N=8, K=8), dict(M=8, N=-1, K=8), dict(M=8, N=8, K=0), dict(M=8, N=8, K=8, batch=0)):
        plan = hb.gemm_plan(kw["M"], kw["N"], kw["K"], batch=kw.get("batch", 1), split_k=1)
        assert plan["rc"] == ASR_E_ARG and hb.gemm_det_split(**kw)["rc"] == ASR_E_ARG, kw
    big = dict(M=64, N=64, K=4096, batch=70000)                                   # grid.y
    assert hb.gemm_plan(64, 64, 4096, batch=70000, split_k=1)["rc"] == ASR_E_SHAPE
    assert hb.gemm_det_split(**big)["rc"] == ASR_E_SHAPE
    assert hb.gemm_det_split(64, 64, 64, arith=7)["rc"] == ASR_E_ARG == hb.gemm_plan(64, 64, 64, arith=7)["rc"]


def test_the_switch_is_off_by_default_and_scoped(hb):
    if os.environ.get("ASR_DETERMINISTIC", "0") != "1":
        assert not hb.is_deterministic()
    old = hb.DETERMINISTIC[0]
    with hb.deterministic():
        assert hb.is_deterministic()
        with hb.deterministic(False):
            assert not hb.is_deterministic()
        assert hb.is_deterministic()
    assert hb.DETERMINISTIC[0] == old


def test_no_side_stream_in_deterministic_mode(hb):
    import ops
    assert ops._SIDE.enabled and (hb.current_arith() & 0xff) != hb.ARITH_F32
    with hb.deterministic(False):
        assert ops._SIDE.usable() and ops._SIDE.usable(0xF0)
    with hb.deterministic():
        assert not ops._SIDE.usable() and not ops._SIDE.usable(0xF0)


def _solver_config(root, **over):
    import yaml
    from dataset import synthetic_utterances
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    vocab = {s: i for i, s in enumerate(["<PAD>", "<BOS>", "<EOS>"] + [chr(ord("a") + i) for i in range(8)] + ["<space>", "<NOISE>"])}
    for name, n, seed in (("train", 6, 1), ("dev", 4, 2)):
        with open(os.path.join(root, name + ".pkl"), "wb") as f:
            pickle.dump(synthetic_utterances(n, 16, len(vocab), 40, seed), f)
    with open(os.path.join(root, "vocab_dict.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(root, "non_lang_syms.pkl"), "wb") as f:
        pickle.dump(["<NOISE>", "<PAD>", "<BOS>", "<EOS>"], f)
    with open(os.path.join(here, "semi-supervised-asr_amd", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(logdir=os.path.join(root, "log"), model_dir=root, model_name="m", load_model_path=os.path.join(root, "m"),
               load_judge_path=os.path.join(root, "m"), dataset_root_dir=root, vocab_path=os.path.join(root, "vocab_dict.pkl"),
               non_lang_syms_path=os.path.join(root, "non_lang_syms.pkl"), labeled_set="train", unlabeled_speech_set="train",
               unlabeled_text_set="train", dev_set="dev", test_set="dev", min_feature_length=4, max_dec_timesteps=8, batch_size=4,
               input_dim=16, enc_hidden_dim=16, enc_n_layers=2, subsample=[2, 2], dec_hidden_dim=16, att_dim=16, att_odim=16,
               conv_channels=2, conv_kernel_size=3, embedding_dim=16, dis_hidden_dim=16, dis_embedding_dim=16)
    cfg.update(over)
    return cfg


def test_solver_refuses_deterministic_with_dp_overlap(hb, tmp_path, monkeypatch):
    import solver as S
    monkeypatch.chdir(str(tmp_path))
    with pytest.raises(ValueError, match="deterministic"):
        S.Solver(_solver_config(str(tmp_path), deterministic=True, dp_overlap=True))
    solver = S.Solver(_solver_config(str(tmp_path), deterministic=True))
    assert solver.deterministic and not hb.is_deterministic(), "the mode is entered per train step, not left switched on"
    assert not S.Solver(_solver_config(str(tmp_path))).deterministic
