"""GPU: LoRA fine-tuning of a Qwen3 ranker -- the live-adapter forward norms q and k (a k_proj adapter's delta included) and the
backward runs lr_launch_qk_norm_bwd behind the attention backward. Loss, gradients and two AdamW steps against the goldens of
tests/gen_goldens_qwen3_train.py (HF Qwen3ForCausalLM with the restated peft layer), live-adapter scores against the merged
inference path, the k_norm margin of k_proj.lora_B's gradient, deterministic mode, the unchanged workspace of a Llama handle,
and the train_ranker.py entry point."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests.gen_goldens_qwen3_train import lora_init, rel

pytestmark = pytest.mark.gpu

SETS = ("qv", "qkvo")
# lr_llama_lora_workspace_bytes (max_loss_rows = 6) and lr_llama_lora_eval_workspace_bytes of a q|v, r = 8 engine on
# tests/golden/llama_lora_train_tiny_hd128.npz's Llama for (max_tokens, max_seqs) = (131, 3), as the commit before the q/k norms
# carved them: a handle without q/k norms keeps its layout and sizes to the byte
LLAMA_WORKSPACE_131_3 = (2189568, 1083904)


def _load(golden_dir, tag):
    from llamarec_amd.synth import synth_qwen3_state

    z = np.load(os.path.join(golden_dir, f"qwen3_lora_train_hd128_gqa_{tag}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_qwen3_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]), qk_norm_spread=float(z["qk_norm_spread"]))
    names = [str(n) for n in z["param_names"]]
    modules = tuple(str(m) for m in z["modules"])
    return z, cfg, sd, names, modules, lora_init(cfg, int(z["weight_seed"]), modules, int(z["lora_r"]))


def _unpack(z, step):
    lens = z[f"step{step}/lens"]
    ids, lab = z[f"step{step}/packed_ids"], z[f"step{step}/packed_labels"]
    cu = np.concatenate([[0], np.cumsum(lens)])
    return ([ids[cu[i]:cu[i + 1]] for i in range(len(lens))], [lab[cu[i]:cu[i + 1]] for i in range(len(lens))])


def _engine(z, cfg, sd, modules, init, **kw):
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    kw.setdefault("dropout", 0.0)
    return LoraTrainEngine(LlamaRanker.from_state_dict(sd, cfg), r=int(z["lora_r"]), alpha=float(z["lora_alpha"]), init=init,
                           target_modules=modules, **kw)


@pytest.mark.parametrize("tag", SETS)
def test_loss_and_lora_gradients_match_reference(golden_dir, tag):
    """bf16 HIP step vs HF's fp32 run, held to test_gpu_llama_train.test_loss_and_lora_gradients_match_reference's bars: 3 % per
    tensor, 1.5 % overall, and three times the archive's own bf16-versus-fp32 gap plus 2e-3."""
    z, cfg, sd, names, modules, init = _load(golden_dir, tag)
    eng = _engine(z, cfg, sd, modules, init)
    assert eng.ranker.family == "qwen3"
    seqs, labels = _unpack(z, 0)
    loss = float(eng.loss_and_grads(seqs, labels))
    got = {k: v.detach().cpu().numpy() for k, v in eng.named(eng.grads).items()}
    per = {n: rel(got[n], z["step0/grad/" + n].astype(np.float64)) for n in names}
    allg = np.concatenate([got[n].ravel() for n in names])
    allr = np.concatenate([z["step0/grad/" + n].ravel() for n in names]).astype(np.float64)
    print(f"{tag}: loss {loss:.5f} vs {float(z['step0/loss']):.5f}; gradient rel err overall {rel(allg, allr):.4f} (the reference's own "
          f"bf16 run {float(z['bf16/grad_rel_all']):.4f}), per tensor {min(per.values()):.4f} .. {max(per.values()):.4f} (the reference's "
          f"{float(z['bf16/grad_rel'].min()):.4f} .. {float(z['bf16/grad_rel'].max()):.4f})")
    assert eng.bad_targets == 0
    assert abs(loss - float(z["step0/loss"])) < 4e-3
    for n in names:
        assert per[n] < 3e-2, (n, per[n])
    assert rel(allg, allr) < 1.5e-2
    assert rel(allg, allr) < 3 * float(z["bf16/grad_rel_all"]) + 2e-3


@pytest.mark.parametrize("tag", SETS)
def test_two_adamw_steps_follow_reference(golden_dir, tag):
    z, cfg, sd, names, modules, init = _load(golden_dir, tag)
    eng = _engine(z, cfg, sd, modules, init)
    lr = 2e-4
    for step in range(2):
        seqs, labels = _unpack(z, step)
        loss = float(eng.loss_and_grads(seqs, labels))
        # test_gpu_lora_modules' bar: 1e-2, or three times what bf16 arithmetic alone does to this loss in the reference plus 4e-3
        ref, ref_bf16 = float(z[f"step{step}/loss"]), float(z["bf16/loss" if step == 0 else "bf16/step1_loss"])
        bar = max(1e-2, 3 * abs(ref_bf16 - ref) + 4e-3)
        print(f"{tag} step {step}: loss {loss:.5f} reference {ref:.5f} its bf16 run {ref_bf16:.5f} bar {bar:.2e}")
        assert abs(loss - ref) < bar, (loss, ref, bar)
        norm = float(eng.apply(lr, float(z[f"step{step}/clip_limit"])))
        assert abs(norm - float(z[f"step{step}/grad_norm"])) < 2e-2 * float(z[f"step{step}/grad_norm"])
        p = eng.named()
        for n in names:
            ref = init[n].astype(np.float64) + z[f"step{step}/update/" + n].astype(np.float64)
            diff = np.abs(p[n].cpu().numpy() - ref)
            g = np.abs(z["step0/grad/" + n])
            if step == 0:
                big = g > 0.05 * g.max()
                assert diff[big].max() < 0.1 * lr, n
            assert diff.max() <= 2.05 * lr * (step + 1), n
            assert diff.mean() < 0.25 * lr, n


def test_k_proj_gradient_passes_through_k_norm(golden_dir):
    """With k_proj adapted, the gradient of k_proj.lora_B is non-zero and more than 10 % (relative L2) from what the generator
    recorded for a model without k_norm (its distance to the reference's is held by the per-tensor bar above)."""
    z, cfg, sd, names, modules, init = _load(golden_dir, "qkvo")
    eng = _engine(z, cfg, sd, modules, init)
    eng.loss_and_grads(*_unpack(z, 0))
    got = {k: v.detach().cpu().numpy() for k, v in eng.named(eng.grads).items()}
    kb = [n for n in names if n.endswith("k_proj.lora_B")]
    assert len(kb) == cfg["num_hidden_layers"]
    for n in kb:
        without = rel(got[n], z["no_k_norm/grad/" + n].astype(np.float64))
        print(f"{n}: |g| {np.linalg.norm(got[n]):.4f}, vs reference {rel(got[n], z['step0/grad/' + n].astype(np.float64)):.4f}, "
              f"vs the model without k_norm {without:.3f}")
        assert np.linalg.norm(got[n]) > 0 and without > 0.1


def test_live_adapter_scores_equal_merged_inference(golden_dir):
    """lr_llama_lora_prefill_verbalize norms q and k through the LoRA forward; the inference path merges the adapters at load and
    norms in the sweep. Same scores to bf16 resolution (test_gpu_llama_train's bar), k_proj's adapter included."""
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, names, modules, init = _load(golden_dir, "qkvo")
    eng = _engine(z, cfg, sd, modules, init)
    seqs, _ = _unpack(z, 0)
    label_ids = np.arange(10, 30, dtype=np.int32)
    live = eng.scores(seqs, label_ids).cpu().numpy()
    weights = {}
    for n in names:
        _, l, proj, ab = n.split(".")
        weights[f"model.layers.{l}.self_attn.{proj}.{ab}.weight"] = init[n]
    merged = LlamaRanker.from_state_dict(sd, cfg, lora=dict(r=int(z["lora_r"]), alpha=float(z["lora_alpha"]), weights=weights))
    ref = merged.prefill_verbalize(seqs, label_ids).cpu().numpy()
    base = LlamaRanker.from_state_dict(sd, cfg).prefill_verbalize(seqs, label_ids).cpu().numpy()
    print(f"live - merged {np.abs(live - ref).max():.4f}, adapter's effect {np.abs(ref - base).max():.4f}")
    assert np.abs(live - ref).max() < 3e-2 * max(1.0, np.abs(ref).max())
    assert np.abs(ref - base).max() > 3 * np.abs(live - ref).max()
    merged_engine = eng.merge_into_base_()
    assert np.abs(merged_engine.prefill_verbalize(seqs, label_ids).cpu().numpy() - ref).max() < 3e-2 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("tag", SETS)
def test_two_deterministic_passes_are_bit_identical(golden_dir, tag):
    z, cfg, sd, names, modules, init = _load(golden_dir, tag)
    seqs, labels = _unpack(z, 0)
    runs = []
    for _ in range(2):
        eng = _engine(z, cfg, sd, modules, init).set_deterministic(True)
        loss = eng.loss_and_grads(seqs, labels)
        runs.append((loss.detach().clone().view(torch.int32), eng.grads.detach().clone().view(torch.int32)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].view(torch.float32).abs().max()) > 0


def test_a_llama_handles_workspace_is_what_it_was(golden_dir):
    from llamarec_amd._lib import lib
    from tests.test_gpu_llama_train import _engine as llama_engine
    from tests.test_gpu_llama_train import _load as llama_load

    z, cfg, sd, names = llama_load(golden_dir, "tiny_hd128")
    eng = llama_engine(z, cfg, sd, names)
    got = lib().lr_llama_lora_workspace_bytes(eng._h, 131, 3, 6)
    ev = lib().lr_llama_lora_eval_workspace_bytes(eng._h, 131, 3)
    print("llama workspace bytes (131, 3, 6):", got, "eval:", ev)
    assert (got, ev) == LLAMA_WORKSPACE_131_3
    # a Qwen3 handle of the same widths needs the pre-norm q | k save buffer on top, per layer
    zq, cq, sq, nq, mods, init = _load(golden_dir, "qv")
    q = _engine(zq, cq, sq, mods, init)
    with_norm = lib().lr_llama_lora_workspace_bytes(q._h, 131, 3, 6)
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    bare_sd = dict({k: v for k, v in sq.items() if "_norm.weight" not in k}, **{"lm_head.weight": sq["model.embed_tokens.weight"]})
    bare = LoraTrainEngine(LlamaRanker.from_state_dict(bare_sd, {k: v for k, v in cq.items() if k != "model_type"}), r=8, alpha=32,
                           dropout=0.0, init=init, target_modules=mods)
    without = lib().lr_llama_lora_workspace_bytes(bare._h, 131, 3, 6)
    save = -(-131 * (4 + 2) * 128 * 2 // 256) * 256
    assert with_norm - without == cq["num_hidden_layers"] * save


def test_train_ranker_synthetic_qwen3_trains_checkpoints_and_scores(tmp_path):
    """`train_ranker.py --synthetic --llm qwen3` runs a few steps, writes checkpoint-N, adapter/ and the metric files, and
    `--eval_only --llm_adapter_path` on the result scores; the four other non-Llama families still exit with eval_only."""
    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    assert pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))["test_users"]
    out = str(tmp_path / "experiments" / "qwen3" / "synthetic")
    flags = ["--dataset_code", "synthetic", "--synthetic", "--llm", "qwen3", "--llm_retrieved_path", lru_root, "--llm_max_history", "5"]
    metrics, overall = train_ranker.main(flags + ["--export_root", out, "--lora_max_steps", "4", "--lora_val_iterations", "2",
                                                  "--lora_save_steps", "2", "--warmup_steps", "1", "--lora_micro_batch_size", "4",
                                                  "--train_batch_size", "8", "--lora_max_val_samples", "16", "--deterministic",
                                                  "--lora_target_modules", "q_proj", "k_proj", "v_proj"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint")) == ["checkpoint-2", "checkpoint-4"]
    for f in ("subset_metrics.json", "overall_metrics.json", os.path.join("adapter", "adapter_model.safetensors"),
              os.path.join("adapter", "adapter_config.json"), os.path.join("checkpoint-4", "optimizer.safetensors")):
        assert os.path.exists(os.path.join(out, f)), f
    assert sorted(json.load(open(os.path.join(out, "adapter", "adapter_config.json")))["target_modules"]) == ["k_proj", "q_proj", "v_proj"]
    scored = str(tmp_path / "scored")
    m2, _ = train_ranker.main(flags + ["--export_root", scored, "--eval_only", "--llm_adapter_path", os.path.join(out, "adapter")])
    assert "test_NDCG@10" in m2 and os.path.exists(os.path.join(scored, "subset_metrics.json"))
    for llm in ("gemma", "gemma2", "phi3", "qwen2"):
        with pytest.raises(SystemExit, match="eval_only"):
            train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", llm, "--llm_retrieved_path", lru_root])
