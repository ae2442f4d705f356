"""Bounds of tests/test_smpl_init_gpu.py.  Fixed by the formats / the project's conventions:"""
SAMPLE_POINT = 1e-6          # points and normals of mp_fit_sample vs the float64 restatement (unit-sized meshes, fp32 round-off)
SAMPLE_CDF_EPS = 1e-6        # a uniform this close to a CDF step may pick the neighbouring face ...
SAMPLE_EXCUSED = 1e-3        # ... for at most this share of the samples
CHI2_LEVEL = 1e-4            # face-selection frequencies vs the exact areas, 10^6 samples, fixed seed
LOSS_REL = 2e-5              # mp_fit_loss vs float64 autograd, relative to the largest entry (the bound mp_loss_fused meets)
STEP_LOSS_REL = 3e-5         # the loss of one fit step / of step 1 vs the torch statement
PARAM_GRAD_REL_L2 = 5e-3     # per-tensor relative L2 of the parameter gradients
F16_PREACT = 454.0           # |z'| the f16 kernels can hold (csrc/mlp_core.hpp)

# ---- measured on MI355X (profiles/smpl_init_fit.txt)
# The fit against the torch restatement of the whole loop (icosphere, 2 048 + 2 048 points, 200 steps, lr 5e-4): held-out mean
# |sdf - exact distance| (4 096 surface + 4 096 box points), 0.1647 before the fit.
#   seed            0         1         2
#   restatement  8.60e-3   1.162e-2  1.039e-2      seed-to-seed spread (max - min) / min = 0.351; gain over "before" 19.2 / 14.2 / 15.9
#   device fit   1.08e-2   1.160e-2  1.013e-2      (a second run of seed 0: 1.13e-2 -- the weight-gradient GEMMs are not run-to-run identical)
#   ratio         1.258     0.999     0.975        largest measured, seed 0 second run: 1.312
# FIT_RATIO_MAX = the largest measured ratio + the restatement's own seed-to-seed spread = 1.312 + 0.351.
# FIT_GAIN_MIN  = the restatement's gain (mean over its three seeds, 16.4) minus the spread of that gain over the seeds (19.2 - 14.2):
#                 from the restatement's numbers alone; the device fit measured 14.2 ... 16.3.
FIT_RATIO_MAX = 1.66
FIT_GAIN_MIN = 11.4
# Person 0 of the synthetic scene fitted to synthetic.closed_body_mesh (24 660 faces) with the DEFAULT FitConfig: held-out |sdf - d|
# on 4 096 surface / 4 096 box points and the distance of the fitted net's extracted level set to the target.  Bounds <= 5x measured:
# measured       2.36e-3           6.86e-3           4.37e-3         2.38e-2         2.49e-3              7.01e-3
BODY = dict(surface_mean=1e-2, surface_max=3e-2, box_mean=2e-2, box_max=1e-1, levelset_mean=1e-2, levelset_max=3e-2)
# Eval frame (1 024 rays, 2 persons, both warm-started from the fitted file) vs the CPU oracle on the device's hit sets: (max, mean),
# <= 5x measured.  Measured: rgb 2.6e-5, 4.9e-6; fg_rgb 2.8e-4, 8.7e-5; acc_map 5.4e-4, 1.7e-4; acc_person 5.4e-4, 8.8e-5; normals
# 1.5e-3, 1.2e-4 -- every one inside tests/tolerances.py EVAL (no ray above 3e-3).  Largest scaled pre-activation of the fitted nets: 111.5.
RENDER = {"rgb_values": (1.2e-4, 2.4e-5), "fg_rgb_values": (1.3e-3, 4e-4), "acc_map": (2.5e-3, 8e-4),
          "acc_person_list": (2.5e-3, 4e-4), "normal_values": (7e-3, 5.5e-4)}
