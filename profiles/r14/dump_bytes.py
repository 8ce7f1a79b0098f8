"""usage: dump_bytes.py ARM_ROOT OUT_DIR -- run every preprocessing entry of the package under ARM_ROOT on fixed inputs
and write the raw output bytes (and the packs' defined bytes) to OUT_DIR, one file each."""
import os
import sys

ARM, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, ARM)
os.makedirs(OUT, exist_ok=True)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import can_distributed_pytorch_amd as pkg  # noqa: E402
assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == ARM, pkg.__file__
from can_distributed_pytorch_amd.data.dataset import density_to_gt  # noqa: E402
from can_distributed_pytorch_amd.ops import _ext  # noqa: E402
from can_distributed_pytorch_amd.ops.conv import dt_code  # noqa: E402
from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_batch, preprocess_packed  # noqa: E402
import test_gpu_crop  # noqa: E402
import test_gpu_scale_crop  # noqa: E402

C = _ext.require()
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def put(name, t):
    t = t.detach().cpu().contiguous()
    with open(os.path.join(OUT, name + ".bin"), "wb") as f:
        f.write(t.view(torch.uint8).numpy().tobytes())


def pack_bytes(packed):
    """The defined bytes of a pack: images | ground truth | descriptors (the alignment gaps are uninitialised)."""
    buf, meta = packed
    n, ho, wo, goff, doff = meta[:5]
    desc = buf[doff:].view(torch.int64).view(n, 8)
    iend = int((desc[:, 0] + desc[:, 1] * desc[:, 2] * desc[:, 3]).max())
    gend = goff + 4 * n * (ho // 8) * (wo // 8)
    assert iend <= goff < iend + 16 and gend <= doff < gend + 16
    return torch.cat([buf[:iend], buf[goff:gend], buf[doff:], torch.tensor(meta, dtype=torch.int64).view(torch.uint8)])


def rgb(rng, h, w, c=3):
    return torch.from_numpy(rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8))


rng = np.random.default_rng(77)
packs = {"hand_crop": test_gpu_crop._hand_pack()[0], "hand_scaled": test_gpu_scale_crop._hand_pack()[0],
         "hand_scaled_big": test_gpu_scale_crop._hand_pack([((71, 131, 3), [(70, 120, 0), (66, 99, 1), (71, 131, 1)])],
                                                           seed=8, crop=(64, 96))[0]}
samples = []
for i, (h, w, c) in enumerate([(77, 101, 3), (72, 96, 3), (79, 103, 1), (72, 100, 4)]):
    dm = rng.random((h, w)).astype(np.float32)
    samples.append((rgb(rng, h, w, c), torch.from_numpy(density_to_gt(dm, h, w, 8, bool(i % 2))), bool(i % 2)))
packs["hand_resize"] = PackedCollate()(samples)
H, W = 384, 512
g1 = torch.from_numpy(rng.random((1, H // 8, W // 8)).astype(np.float32))
packs["b8_resize"] = PackedCollate()([(rgb(rng, H + 5 + i % 3, W + 7 - i % 2), g1, bool(i % 2)) for i in range(8)])
packs["b8_crop"] = PackedCollate(crop=(H, W))(
    [(rgb(rng, 500, 700), g1[None], torch.tensor([[int(rng.integers(0, 117)), int(rng.integers(0, 189)), i % 2]]))
     for i in range(8)])
items = []
for i in range(8):
    sh, sw = int(rng.integers(288, 501)), int(rng.integers(384, 701))
    items.append((rgb(rng, 500, 700), g1[None],
                  torch.tensor([[int(rng.integers(0, 501 - sh)), int(rng.integers(0, 701 - sw)), i % 2, sh, sw]])))
packs["b8_scaled"] = PackedCollate(crop=(H, W), crop_scale=True)(items)

ap = AheadPrep("cuda")
for name, packed in packs.items():
    put("pack_" + name, pack_bytes(packed))
    for dn, dt in DT.items():
        x4, gt = preprocess_packed(packed, "cuda", dtype=dt)
        torch.cuda.synchronize()
        put(f"x4_{name}_{dn}", x4)
        put(f"gt_{name}_{dn}", gt)
    a4, ag = ap.ready(ap.issue(packed))
    torch.cuda.synchronize()
    put(f"x4_{name}_ahead_bf16", a4)

# the per-sample entries (C.preprocess_image, C.preprocess_density)
for (h, w, c) in [(77, 101, 3), (50, 70, 1), (72, 100, 4)]:
    img, dm = rgb(rng, h, w, c), torch.from_numpy(rng.random((h, w)).astype(np.float32))
    for fl in (0, 1):
        for dn, dt in DT.items():
            x4, gt = preprocess_batch([img], [dm], [bool(fl)], "cuda", dtype=dt)
            torch.cuda.synchronize()
            put(f"image_{h}x{w}x{c}_f{fl}_{dn}", x4)
            put(f"density_{h}x{w}_f{fl}_{dn}", gt)
dm = torch.from_numpy(rng.random((23, 31)).astype(np.float32))            # a density of another size than the image
put("density_23x31_to_10x14", preprocess_batch([rgb(rng, 80, 112)], [dm], [True], "cuda")[1])

# synth_render on a fixed density (no splat atomics ahead of it)
n, h, w = 2, 128, 192
dens = (torch.from_numpy(rng.random((n, h, w)).astype(np.float32)) ** 8).cuda()
noise = torch.from_numpy(rng.random((n, 3, h // 16, w // 16)).astype(np.float32)).cuda()
st = _ext.stream_ptr(torch.device("cuda"))
for dn, dt in DT.items():
    x4 = torch.empty(n, h, w, 4, dtype=dt, device="cuda")
    gt = torch.empty(n, 1, h // 8, w // 8, device="cuda")
    dmax = torch.empty(n, device="cuda")
    C.synth_render(dens.data_ptr(), noise.data_ptr(), dmax.data_ptr(), x4.data_ptr(), gt.data_ptr(), n, h, w,
                   dt_code(dt), st)
    torch.cuda.synchronize()
    put(f"synth_x4_{dn}", x4)
    put(f"synth_gt_{dn}", gt)
    put(f"synth_dmax_{dn}", dmax)
print("dumped", len(os.listdir(OUT)), "files to", OUT, "from", ARM)
