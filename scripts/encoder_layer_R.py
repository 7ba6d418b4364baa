#!/usr/bin/env python3
"""|mean| / std (R) of every pre-norm convolution output of the Patchifier's
fnet, per channel, in fp64 on the CPU -- the quantity that decides how much of
the instance-norm variance the one-pass (sum, sum of squares) statistics of
csrc/encoder.hip lose (profiles/encoder_layers/NOTES.md).

Weights: the random initialisation the encoder tests use (Patchifier(3) after
torch.manual_seed(0)) and the seeded weights of tests/golden/encoder_ref.npz.
Frames: the tests' "texture" and "noise" frames and a flat frame (128, +-1 on
1 % of the pixels), at 384 x 512 and 100 x 134.  Prints a markdown table.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "wild-video-3d-reconstruction_amd"), os.path.join(REPO, "tests"),
          os.path.join(REPO, "tests", "golden")):
    sys.path.insert(0, p)

import encoder_layers_ref as R  # noqa: E402
import net_inputs as NI  # noqa: E402


def frames(H, W):
    from dpvo.synthetic import image_stream
    g = torch.Generator().manual_seed(1)
    noise = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    texture = next(iter(image_stream(1, H, W, seed=1, device="cpu")))[1]
    flat = torch.full((3, H, W), 128, dtype=torch.int16)
    r = torch.rand(3, H, W, generator=g)
    flat = (flat + (r < 0.005).short() - (r > 0.995).short()).to(torch.uint8)
    return {"texture": texture, "noise": noise, "flat": flat}


def nets():
    from dpvo.extractor import BasicEncoder4
    from dpvo.net import Patchifier
    torch.manual_seed(0)
    yield "tests (seed 0)", Patchifier(3).fnet.double().eval()
    f = np.load(os.path.join(REPO, "tests", "golden", "encoder_ref.npz"))
    fnet = BasicEncoder4(128, "instance")
    params = NI.make_params(str(f["fspec"]), NI.ENCODER_SEED)
    fnet.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    yield "golden (seed 41)", fnet.double().eval()


def main():
    rows, top = [], 0.0
    for wname, enc in nets():
        for H, W in ((384, 512), (100, 134)):
            for fname, u8 in frames(H, W).items():
                seen = {}
                with torch.no_grad():
                    R.encoder_chain(enc, u8, round16=False,
                                    on_layer=lambda name, y: seen.__setitem__(name, R.channel_R(y).max().item()))
                worst = max(seen, key=seen.get)
                top = max(top, seen[worst])
                rows.append((wname, f"{H}x{W}", fname, seen))
    names = list(rows[0][3])
    print("| weights | frame | kind | " + " | ".join(n.replace("|", "+") for n in names) + " | max |")
    print("|---|---|---|" + "---|" * (len(names) + 1))
    for wname, size, fname, seen in rows:
        print(f"| {wname} | {size} | {fname} | " + " | ".join(f"{seen[n]:.2f}" for n in names) +
              f" | {max(seen.values()):.2f} |")
    print(f"\nlargest per-channel R: {top:.2f}")


if __name__ == "__main__":
    main()
