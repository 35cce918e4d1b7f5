"""SHA-256 digests of the head's and the front's trainer state after three rounds of forward_backward / clip(0.5) / step, for decoders
WITHOUT cross-attention: what a change to the shared trainer layer must leave bit for bit (profiles/r11/README.md describes the items).

    cd <root of the tree to be measured> && python <this file> > digests.txt

The package is imported from the current directory, so the same file measures a checkout of another commit (built there) when it is
run from that checkout's root; two trees agree when their outputs are identical (`cmp`)."""
import contextlib
import hashlib
import io
import os
import sys

sys.path.insert(0, os.getcwd())
import torch
from vae_tagger_amd import synth
from vae_tagger_amd.train import DecoderTrainer, HeadTrainer
from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
DEV = "cuda:0"
def latent_input(shape, seed):
    return 0.1159 + 0.8 * torch.randn(shape, generator=torch.Generator().manual_seed(seed))
def labels(B, seed):
    return (torch.rand(B, 11, generator=torch.Generator().manual_seed(seed)) < 0.3).to(torch.uint8)
def quiet(make):
    with contextlib.redirect_stdout(io.StringIO()):          # (the decoders' constructors print their configuration)
        return make()
def dig(name, t):
    print(name, hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest())
for plain in (True, False):
    d = quiet(lambda: ClassificationDecoder(16, 16, 16, 11) if plain else AttentionClassificationDecoder(16, 16, 16, 11))
    d.load_state_dict(synth.synth_state_dict((synth.plain_decoder_manifest if plain else synth.attention_decoder_manifest)(11), seed=1), strict=False)
    d = d.to(DEV).eval()
    tr = HeadTrainer(d, seed=3)
    for s in range(3):
        tr.forward_backward(tr.features(latent_input((3, 16, 9, 20), 100 + s).to(DEV)), labels(3, 110 + s).to(DEV), train=True, step=s)
        tr.clip(0.5); tr.step(1e-2, 1e-6)
    tag = "head/" + ("plain" if plain else "attention")
    dig(tag + " state", tr.state_bytes()); dig(tag + " losses", tr.losses()); dig(tag + " forward", tr.forward(tr.features(latent_input((3, 16, 9, 20), 120).to(DEV))))
for name, cfg in (("sp-sa8", (1, 1, 8)), ("sp-sa2", (1, 1, 2)), ("sp", (1, 0, 8)), ("sa8", (0, 1, 8)), ("compress", (0, 0, 8))):
    d = quiet(lambda: AttentionClassificationDecoder(16, 16, 16, 11, bool(cfg[0]), bool(cfg[1]), False, cfg[2]))
    d.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(11, 16, bool(cfg[0]), bool(cfg[1]), False), seed=1), strict=False)
    d = d.to(DEV).eval()
    tr = DecoderTrainer(d, attention_dropout=0.1, seed=3)
    for s in range(3):
        tr.forward_backward(latent_input((3, 16, 9, 20), 200 + s).to(DEV), labels(3, 210 + s).to(DEV), train=True, step=s)
        tr.clip(0.5); tr.step(1e-2, 1e-6)
    lat = latent_input((3, 16, 9, 20), 220).to(DEV)
    dig(f"full/{name} front", tr.front.state_bytes()); dig(f"full/{name} head", tr.head.state_bytes()); dig(f"full/{name} losses", tr.losses())
    dig(f"full/{name} forward", tr.forward(lat)); tr.commit(); dig(f"full/{name} committed", d(lat))
