"""CPU side of the fused residual LayerNorm path (ops/residual_ln.py): without
a GPU the model takes the unfused path, and the layer keeps its interface."""
import torch


def test_falls_back_without_gpu(monkeypatch):
    from oktopk_amd.models.bert import BertConfig, BertLayer
    from oktopk_amd.ops.residual_ln import residual_ln_available

    cfg = BertConfig(hidden_size=768, num_attention_heads=12, intermediate_size=64,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    layer = BertLayer(cfg)
    x = torch.randn(2, 4, 768)
    monkeypatch.setenv("OKTOPK_FUSED_RESIDUAL_LN", "0")
    off = layer(x)
    monkeypatch.setenv("OKTOPK_FUSED_RESIDUAL_LN", "1")
    assert not residual_ln_available(x, x.clone(), layer.ln1)
    on = layer(x)
    assert torch.equal(on, off)
    on.sum().backward()
    assert layer.ln1.weight.grad is not None


def test_layer_interface_unchanged():
    from oktopk_amd.models.bert import BertConfig, BertForPreTraining

    cfg = BertConfig(vocab_size=64, hidden_size=32, num_hidden_layers=2,
                     num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=16)
    model = BertForPreTraining(cfg)
    keys = set(model.state_dict())
    for i in range(2):
        for name in ("ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias",
                     "attn.qkv.weight", "fc1.weight", "fc2.bias"):
            assert f"bert.layer.{i}.{name}" in keys
    # pipeline stages slice bert.layer and call each layer as layer(x, mask) -> x
    x = torch.randn(2, 4, 32)
    for lyr in model.bert.layer[1:2]:
        out = lyr(x, None)
    assert isinstance(out, torch.Tensor) and out.shape == x.shape
