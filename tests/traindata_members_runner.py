"""One run of an EvalNet training-data writer at toy size (a plain module with main(), started by tests/test_gpu_traindata_members.py
as a fresh child process: IMK_TRAINDATA_POOLED and IMK_INFER_BATCH are read once per process).

    python tests/traindata_members_runner.py binary|multi|hela DATA_DIR OUT_DIR

5 pool models, 12 images, 2 loops, a fixed seed.  The data set is made from a seed if DATA_DIR does not hold it yet.  Prints one JSON
line: how often the pool's and the group ensembles' run() were called."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_MODELS, N_IMAGES, N_LOOPS, SEED = 5, 12, 2, 1234
# kind -> (h, w, c, k, alpha, head)
KINDS = {"binary": (32, 32, 3, 1, 0.5, "sigmoid"), "multi": (32, 48, 3, 9, 0.5, "softmax"), "hela": (32, 32, 1, 3, 1.0, "sigmoid")}


def make_data(kind, data_dir):
    import numpy as np
    from inconsistencymasks_amd import functions as F
    h, w, c, k, _, _ = KINDS[kind]
    rng = np.random.default_rng(SEED)
    yy, xx = np.mgrid[0:h, 0:w]
    subs = ("brightfield", "alive", "dead", "mod_position") if kind == "hela" else ("images", "masks")
    for s in subs:
        os.makedirs(os.path.join(data_dir, s), exist_ok=True)
    for i in range(N_IMAGES):
        name = f"img_{i:03d}.png"
        img = (127 + 80 * np.sin(xx / (3.0 + i))[..., None] * np.cos(yy / 5.0)[..., None] + rng.integers(-30, 30, (h, w, c))).clip(0, 255)
        blob = ((yy - h / 2) ** 2 + (xx - w / 3 - i) ** 2) < (6 + i % 4) ** 2
        if kind == "hela":
            F.write_png(os.path.join(data_dir, "brightfield", name), img.astype(np.uint8))
            F.write_png(os.path.join(data_dir, "alive", name), blob.astype(np.uint8) * 255)
            F.write_png(os.path.join(data_dir, "dead", name), (~blob & (xx > w // 2)).astype(np.uint8) * 255)
            F.write_png(os.path.join(data_dir, "mod_position", name), (blob & (yy % 4 == 0) & (xx % 4 == 0)).astype(np.uint8) * 255)
        else:
            F.write_png(os.path.join(data_dir, "images", name), img.astype(np.uint8))
            mask = blob.astype(np.uint8) * 255 if kind == "binary" else ((xx // 6 + yy // 8 + i) % k).astype(np.uint8)
            F.write_png(os.path.join(data_dir, "masks", name), mask)


def main(argv):
    kind, data_dir, out_dir = argv[1:4]
    import torch
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd.unet import UNet
    from tests.test_gpu_unet import randomize_bn
    h, w, c, k, alpha, head = KINDS[kind]
    if not os.path.isdir(data_dir):
        make_data(kind, data_dir)
    models = []
    for j in range(N_MODELS):
        m = UNet(h, w, c, k, alpha, head, seed=301 + j)
        m.load_state_dict(randomize_bn(m.state_dict(), 401 + j))
        models.append(m)
    calls = {"pool": 0, "ensemble": 0}

    def counted(cls, key):
        run = cls.run

        def wrapper(self, *a, **kw):
            calls[key] += 1
            return run(self, *a, **kw)
        cls.run = wrapper
    counted(F.PoolIM, "pool")
    counted(F.EnsembleIM, "ensemble")
    if kind == "binary":
        F.create_training_data_evalnet_im_binary(models, h, w, c, os.path.join(data_dir, "images"), os.path.join(data_dir, "masks"), out_dir,
                                                 N_LOOPS, seed=SEED)
    elif kind == "multi":
        F.create_training_data_evalnet_miou_im_multiclass(models, h, w, c, k, os.path.join(data_dir, "images"),
                                                          os.path.join(data_dir, "masks"), out_dir, N_LOOPS, seed=SEED)
    else:
        F.create_training_data_evalnet_miou_im_hela(models, h, w, c, data_dir, out_dir, N_LOOPS, seed=SEED)
    F.flush_writes(all_threads=True)
    torch.cuda.synchronize()
    print(json.dumps({"pool_calls": calls["pool"], "ensemble_calls": calls["ensemble"], "infer_batch": F.INFER_BATCH}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
