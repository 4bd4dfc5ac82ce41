#!/usr/bin/env python3
"""Generate tests/golden/nllb_padded_*.npz: the REFERENCE's own NLLB block (moe_infinity/models/nllb_moe.py) run on CPU
with a padding mask, the way HF's NllbMoeEncoderLayer / NllbMoeDecoderLayer call it (``self.ffn(hidden_states,
attention_mask)``).

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout (as oracle/gen_golden.py, whose importer, FakeDispatcher and
transformers-5.15 adaptations it reuses unchanged); the fixtures it writes are committed.  Re-run:
    python tools/gen_golden_padded.py

The masks are HF's additive 4-D attention masks (0 = attend, the dtype's minimum = masked key):
  * enc_*: an encoder batch with ragged lengths, mask [B, 1, S, S] with padded keys masked (both
    normalize_router_prob_before_dropping settings);
  * dec:   one decoder step of B sequences, mask [B, 1, 1, S_kv]; route_tokens keeps the last B entries of the flattened
    last query rows (HF's quirk, reproduced, not corrected).
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.gen_golden import OUT, FakeDispatcher, _NoCuda, import_reference, make_executor, npf  # noqa: E402
from oracle.synth import acts, checksum, make_weights  # noqa: E402


def additive_mask(keep_keys: torch.Tensor, q_len: int, dtype=torch.float32) -> torch.Tensor:
    """[B, S_kv] bool (True = real key) -> HF additive mask [B, 1, q_len, S_kv]"""
    b, skv = keep_keys.shape
    m = torch.zeros((b, 1, q_len, skv), dtype=dtype)
    m.masked_fill_(~keep_keys[:, None, None, :], torch.finfo(dtype).min)
    return m


def gen(mods, name, b, s, h, f, e, seed, mask4d, dtype=torch.bfloat16, norm_before=False):
    from transformers import NllbMoeConfig

    cfg = NllbMoeConfig(d_model=h, encoder_ffn_dim=f, decoder_ffn_dim=f, num_experts=e, encoder_layers=2,
                        decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4, vocab_size=32,
                        expert_capacity=64, router_dtype="float32", second_expert_policy="all",
                        normalize_router_prob_before_dropping=norm_before, batch_prioritized_routing=False,
                        moe_eval_capacity_token_fraction=1.0, moe_token_dropout=0.2, activation_dropout=0.0,
                        router_ignore_padding_tokens=False)
    blk = mods["nllb_moe"].SyncNllbMoeSparseMLP(cfg, f).to(dtype).eval()
    gate, experts, _ = make_weights("nllb", h, f, e, seed, dtype, gate_std=0.5)
    with torch.no_grad():
        blk.router.classifier.weight.copy_(gate)
        for i, (w1, b1, w2, b2) in enumerate(experts):
            ex = blk.experts[f"expert_{i}"]
            ex.fc1.weight.copy_(w1)
            ex.fc1.bias.copy_(b1)
            ex.fc2.weight.copy_(w2)
            ex.fc2.bias.copy_(b2)
    blk.layer_id = 0

    def nllb_expert(i):  # as oracle/gen_golden.py: matmul, then bias add (core/parallel/expert_module.cpp:88-93)
        ex = blk.experts[f"expert_{i}"]
        return lambda xx: torch.matmul(torch.relu(torch.matmul(xx, ex.fc1.weight.t()) + ex.fc1.bias),
                                       ex.fc2.weight.t()) + ex.fc2.bias

    blk.expert_executor = make_executor(mods, FakeDispatcher(nllb_expert))
    x = acts(b * s, h, dtype, 2024 + seed).reshape(b, s, h)
    orig_router_fwd = blk.router.forward
    # 4.37 semantics (as oracle/gen_golden.py): the router flattened [B,S,H] -> [B*S,H] itself and returned (top_1_mask, probs)
    blk.router.forward = lambda hs, pm=None: orig_router_fwd(hs.reshape(-1, hs.shape[-1]), pm)[:2]
    with _NoCuda(), torch.no_grad():
        out, (router_probs, top1) = blk.forward(x, mask4d)
    real = (router_probs.reshape(b * s, e) != 0).any(-1)
    np.savez_compressed(os.path.join(OUT, name), x=npf(x), out=npf(out), router_probs=npf(router_probs), top1=npf(top1),
                        padding_mask=npf(mask4d), meta=np.array([b, s, h, f, e, seed, int(norm_before)]),
                        wsum=checksum(gate, experts))
    print(name, "ok", out.float().abs().mean().item(), "routed tokens", int(real.sum()), "of", b * s)


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.cuda.device_count = lambda: 1  # as oracle/gen_golden.py: dispatch_local does expert_id % device_count
    mods = import_reference()
    # encoder batch: B = 4, S = 12, lengths 12 / 9 / 5 / 1 (right-padded, as NLLB's tokenizer pads)
    lengths = torch.tensor([12, 9, 5, 1])
    keep = torch.arange(12)[None, :] < lengths[:, None]
    enc_mask = additive_mask(keep, 12)
    gen(mods, "nllb_padded_enc_bf16.npz", 4, 12, 256, 512, 16, 31, enc_mask)
    gen(mods, "nllb_padded_enc_norm_before_bf16.npz", 4, 12, 256, 512, 16, 32, enc_mask, norm_before=True)
    # decoder step: B = 8 sequences of one new token each, 10 key positions; the last 8 entries of the flattened
    # last-query rows are sequence 7's keys 2..9 (keys 6..9 masked)
    keep_dec = torch.ones((8, 10), dtype=torch.bool)
    keep_dec[7, 6:] = False
    keep_dec[3, 8:] = False  # (not reached by the reduction: only the last nb_tokens entries count)
    gen(mods, "nllb_padded_dec_bf16.npz", 8, 1, 256, 512, 16, 33, additive_mask(keep_dec, 1))


if __name__ == "__main__":
    main()
