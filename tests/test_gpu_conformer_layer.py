"""GPU: the conformer layer that engine.W2vBertEncoder and engine.ConformerSpeechEncoder share (engine._ConformerLayers), stated as the
launches it records.  The literal lists below are the command lists of the commit before the two encoders were put on one layer host,
printed from its tapes for the same two utterances: the shared loop must record the same ops in the same order, with the hidden-state
marks at the same places, and as many commands in all."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fixture -> (commands in front of states[0], commands of the whole forward, the first layer, the last layer), from the parent's tapes
# for the fixture's first two utterances.  The relative type's three GEMMs in a row are the packed projection and two 256-row chunks of
# P = linear_pos(pe) (utterances up to 256 frames); the conformer family's last layer ends with encoder.layer_norm.
CASES = {
    "TINY_W2V_BERT": ("tiny_w2v_bert_d128h2", 3, 39,
                      ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "GEMM", "RELKEY_TABLE", "ATTENTION_RK", "GEMM", "LAYERNORM", "GEMM",
                       "CONFORMER_CONV", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM"],
                      ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "GEMM", "RELKEY_TABLE", "ATTENTION_RK", "GEMM", "LAYERNORM", "GEMM",
                       "CONFORMER_CONV", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM"]),
    "TINY_W2V_CONFORMER_ROPE": ("tiny_w2v_conformer_rope", 10, 49,
                                ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "ROPE_ROWS", "GEMM", "GEMM", "ATTENTION", "GEMM", "LAYERNORM",
                                 "GEMM", "CONFORMER_CONV_BN", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM"],
                                ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "ROPE_ROWS", "GEMM", "GEMM", "ATTENTION", "GEMM", "LAYERNORM",
                                 "GEMM", "CONFORMER_CONV_BN", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "LAYERNORM"]),
    "TINY_W2V_CONFORMER_REL": ("tiny_w2v_conformer_rel", 10, 51,
                               ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "GEMM", "GEMM", "GEMM", "RELPOS_BIAS", "ATTENTION_RB", "GEMM",
                                "LAYERNORM", "GEMM", "CONFORMER_CONV_BN", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM"],
                               ["LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "GEMM", "GEMM", "GEMM", "RELPOS_BIAS", "ATTENTION_RB", "GEMM",
                                "LAYERNORM", "GEMM", "CONFORMER_CONV_BN", "GEMM", "LAYERNORM", "GEMM", "SWISH_ROWS", "GEMM", "LAYERNORM", "LAYERNORM"]),
}


@pytest.mark.parametrize("gname", list(CASES))
def test_the_layer_records_the_launches_it_recorded_before(golden_dir, gname):
    import os
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import build_encoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    if gname == "TINY_W2V_BERT":
        import w2vbert_ref as R
    else:
        import w2vconf_ref as R
    tag, front, total, first, last = CASES[gname]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    lengths = [int(n) for n in gold["lengths"]][:2]
    waves = [R.synth_wave(int(gold[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
    enc = build_encoder(geo, synthetic_state_dict(geo, int(gold["seed"])), DEV, "f16x")
    hs = enc.forward(enc.upload(waves), lengths)
    torch.cuda.synchronize()
    assert hs.take_range_bits() == 0
    tape = enc.recorded_tape(lengths, 0)
    names = {v: k[3:] for k, v in vars(_lib).items() if k.startswith("OP_")}
    ops = [names[tape.cmds[i].op] for i in range(tape.n)]
    L = geo.num_layers
    print(f"CONFORMER LAYER {gname} lengths {lengths}: {tape.n} commands, marks {dict(tape.marks)}")
    print(f"CONFORMER LAYER {gname} first layer {ops[tape.marks[0]: tape.marks[1]]}")
    print(f"CONFORMER LAYER {gname} last layer {ops[tape.marks[L - 1]: tape.marks[L]]}")
    assert L >= 2 and sorted(tape.marks) == list(range(L + 1))
    assert tape.marks[0] == front
    assert ops[tape.marks[0]: tape.marks[1]] == first
    assert ops[tape.marks[L - 1]: tape.marks[L]] == last
    assert tape.marks[L] == tape.n == total
