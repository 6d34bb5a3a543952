"""CPU stand-ins for the resume tests (tests/test_resume_host.py, tests/test_resume_gloo.py): an engine with the surface
LoraRankerTrainer uses -- flat params / m / v, the two counters, state_dict / load_state_dict, a step in which the moments
AND the counters matter -- and a sample source that draws from its generator on every __getitem__."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

N = 4


class FakeEngine:
    def __init__(self, r=8, target_modules=("q_proj", "v_proj")):
        self.r, self.target_modules = r, tuple(target_modules)
        self.params = torch.zeros(N, dtype=torch.float32)
        self.grads = torch.zeros(N, dtype=torch.float32)
        self.m, self.v = torch.zeros(N, dtype=torch.float32), torch.zeros(N, dtype=torch.float32)
        self.steps = self.passes = 0
        self.device = torch.device("cpu")
        self.seen = []          # per pass: [(sample index token, drawn token), ...]

    def loss_and_grads(self, seqs, labels, grad_scale=1.0, accumulate=False):
        self.passes += 1
        g = torch.tensor([[float(s.sum()) % 7, float(len(s)), float(s[2]) % 11, 1.0] for s in seqs], dtype=torch.float32).mean(0)
        g = g * (1.0 + 0.125 * (self.passes % 5))                    # "dropout": the pass counter enters the gradient
        self.grads = self.grads + grad_scale * g if accumulate else grad_scale * g
        self.seen.append([(int(s[1]), int(s[2])) for s in seqs])
        return torch.tensor(float(g[0]))

    def apply(self, lr, max_grad_norm=1.0):
        self.m = 0.5 * self.m + self.grads
        self.v = 0.75 * self.v + self.grads * self.grads
        self.steps += 1
        self.params = self.params - lr * self.m / (self.v.sqrt() + 1.0) / (1.0 - 0.5 ** self.steps)   # "bias correction"
        return torch.tensor(0.0)

    def layout(self):
        return dict(r=self.r, target_modules=list(self.target_modules), n_params=N)

    def state_dict(self):
        return dict(params=self.params.clone(), exp_avg=self.m.clone(), exp_avg_sq=self.v.clone(), optimizer_steps=self.steps,
                    passes=self.passes, **self.layout())

    def load_state_dict(self, sd):
        from llamarec_amd.rank_train import check_layout

        check_layout(self.layout(), sd)
        self.params, self.m, self.v = sd["params"].clone(), sd["exp_avg"].clone(), sd["exp_avg_sq"].clone()
        self.steps, self.passes = int(sd["optimizer_steps"]), int(sd["passes"])
        return self

    def export(self, buf=None):
        return {"flat": (self.params if buf is None else buf).clone()}

    def import_flat(self, tensors):
        return tensors["flat"].clone()

    def save_adapter(self, path, base_model=""):
        from safetensors.torch import save_file

        os.makedirs(path, exist_ok=True)
        json.dump({"r": self.r, "target_modules": list(self.target_modules)}, open(os.path.join(path, "adapter_config.json"), "w"))
        save_file(self.export(), os.path.join(path, "adapter_model.safetensors"))


class FakeSamples:
    """36 samples; token 1 names the sample, token 2 is drawn from `rng` when the sample is built."""
    tokenizer = type("T", (), {"eos_token_id": 2})()

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def _draw(self):
        return int(self.rng.randint(0, 500))

    def __len__(self):
        return 36

    def __getitem__(self, i):
        ids = [1, 100 + i, 200 + self._draw()] + [7] * (3 + i % 5) + [30, 2]
        return {"input_ids": ids, "attention_mask": [1] * len(ids), "labels": [-100] * (len(ids) - 2) + ids[-2:]}


class FakeSamplesHiddenRng(FakeSamples):
    """The same source with its generator where the trainer does not look: nothing of it is saved or restored."""

    def __init__(self, seed):
        self._rng = np.random.RandomState(seed)

    def _draw(self):
        return int(self._rng.randint(0, 500))


def lora_args(micro=4, batch=8, **kw):
    """6 steps, validation and a checkpoint every 2; 36 samples / 8 per step = 4 steps per epoch, so step 4 ends epoch 0."""
    a = dict(lora_micro_batch_size=micro, train_batch_size=batch, lora_max_steps=6, lora_num_epochs=1, warmup_steps=2,
             lora_lr=0.1, lora_val_iterations=2, lora_val_delay=0, lora_early_stopping_patience=20,
             rerank_best_metric="NDCG@10", seed=3, llm_max_text_len=64, lora_token_budget=0, lora_save_steps=2,
             lora_save_total_limit=3, resume_from_checkpoint=None)
    a.update(kw)
    return SimpleNamespace(**a)


def make_trainer(args, root, samples=None, engine=None, rank=0, world=1, log=None):
    from llamarec_amd.rank_train import LoraRankerTrainer

    eng = engine or FakeEngine()
    tr = LoraRankerTrainer(args, eng, samples or FakeSamples(11 + rank), [0], None, root, rank, world,
                           log=log or (lambda *a: None))
    # a validation metric that rises and falls with the parameters: best_state / bad_evals both move
    tr.evaluate = lambda: {"NDCG@10": float(torch.sin(40.0 * eng.params.sum()))}
    return tr, eng
