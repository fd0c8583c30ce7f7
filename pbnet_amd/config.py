"""The cfg contract PBNet reads (/root/reference/config/config.py:10-67, config_test.py): field names and defaults
only -- the reference's argparse CLI itself is outside the hot path."""
from types import SimpleNamespace

TRAIN_DEFAULTS = dict(task="train", manual_seed=22, voxel_size=0.02, scale_size=1, sem_num=20, batch_size=4,
                      batch_size_v=1, cluster_epoch=128, min_pts=31, radius=0.04, method=0, fg_thresh=0.95,
                      bg_thresh=0.20, TEST_NMS_THRESH=0.10, TEST_SCORE_THRESH=0.07, TEST_NPOINT_THRESH=101,
                      max_crop_p=300000, min_crop_p=50000,
                      # the training program's own fields (config.py:16-40), read by pbnet_amd.train_epoch / pbnet_amd.optim
                      epochs=520, save_freq=4, logpath="./log/config_1/", lr=0.001, optimizer="Adam", step_epoch=50,
                      momentum=0.9, weight_decay=0.0001,
                      native_losses=False,      # not the reference's: losses through csrc/losses.hip (pbnet_amd/losses.py)
                      device_meters=False,      # not the reference's: model_fn leaves the logged terms on the device
                      native_optimizer=False,   # not the reference's: optim.build_optimizer builds pbnet_amd.optim's classes
                      device_post=False,        # not the reference's: ValidationEpoch refines through refine_instances_device
                      device_ap=False,          # not the reference's: ValidationEpoch associates on the device as well (needs
                                                # device_post): evaluate.AssociationLog, read back once by finish()
                      device_ap_table=False)    # not the reference's: finish() matches and integrates on the device too (needs
                                                # device_ap): evaluate.APTable reads the log where it lies
TEST_OVERRIDES = dict(task="test", batch_size=1, cluster_epoch=-1)


def get_config(test=False, **overrides):
    cfg = dict(TRAIN_DEFAULTS)
    if test:
        cfg.update(TEST_OVERRIDES)
    cfg.update(overrides)
    return SimpleNamespace(**cfg)
