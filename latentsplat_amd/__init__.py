"""latentsplat_amd — MI355X-native Gaussian-splat rasterizer path of latentSplat.

Only what the hot path needs: ``csrc/`` (HIP kernels + C ABI), ``rasterizer`` (drop-in
``GaussianRasterizer`` API + batched multi-view op), ``decoder`` (mirror of the reference's
``src/model/decoder`` surface), ``gaussian_adapter`` / ``sh_rotate`` (the encoder's adapter tail:
geometry and SH coefficient rotation), ``depth_head`` (the encoder's depth logits to the adapter's
depths and opacities; the op itself is ``latentsplat_amd.depth_head.depth_head``), ``ply_export`` / ``ply_import`` (3DGS
``.ply`` files out and in), ``scene_model`` (a trainable 3DGS scene: raw parameters activated in HIP), ``density`` (its adaptive density control: clone, split, prune in HIP), ``mcmc`` (the MCMC strategy: relocate dead Gaussians, grow to a cap, covariance-shaped noise, in HIP), ``filter3d`` (the 3D smoothing filter of Mip-Splatting: the sampling-rate bound per Gaussian and the filtered activation, in HIP), ``knn`` (exact 3-nearest-neighbour distances in HIP: the point-cloud initialisation of a scene), ``optim`` (its Adam step fused into one HIP launch, with a visibility-sparse mode), ``losses`` (the 3DGS photometric loss, L1 + D-SSIM,
and the SSIM metric in HIP), ``bilagrid`` (bilateral-grid appearance compensation between render and loss: per-image grids of
colour affines sliced by position and luminance, and their total variation, in HIP), ``transform`` (similarity transforms of a
scene: positions, quaternions, log-scales and every SH band of the view-dependent colour in one HIP pass; posed parts, merge), ``pose`` (the same transforms as learnable quaternions, translations and log-scales: the pose gradient of a scene's rigid parts in one HIP pass, reduced per part without atomics), ``vq`` (codebook compression of a scene: weighted k-means with a fused distance-and-argmin on the f32 matrix
instruction and a bit-reproducible float64 centroid update, in HIP; quantised scenes in and out of one compressed file), ``normals`` (the depth-normal consistency regulariser: per-view normals of the Gaussians and the fused image-space loss against the normals of the rendered depth, in HIP), ``mesh`` (mesh extraction: rendered depth fused into a
truncated signed distance volume in one pass over the volume per batch of views, and marching tetrahedra, in HIP; mesh ``.ply``
files; connected components and the cleanup that keeps the largest clusters), ``nn`` (the exact nearest neighbour of one
cloud's points in another: a persistent index over a reference cloud, in HIP), ``mesh_eval`` (what scores a mesh against a
ground-truth cloud: accuracy, completeness, Chamfer, precision / recall / F-score, and an area-weighted mesh sampler), ``images`` (photographs
resampled onto the rasterizer's centred, distortion-free camera at the training resolution, with a coverage map, in HIP),
``capture`` (a photographed capture: the COLMAP sparse model through a strict host reader, prepared targets, a train / test
split, camera tables and the initial scene), ``depth_sup`` (depth supervision for captures: sparse-point and monocular-prior
inverse-depth targets, and the fused inverse-depth L1 loss in HIP), ``distortion`` (the depth distortion regulariser: pivoted
depth moments of the Gaussians per view and the fused image-space pair term A M2 - M1^2, in HIP) and ``synthetic`` (seeded scenes for tests / bench).
"""
__version__ = "0.1.0"

_LAZY = {"rotate_sh": "sh_rotate", "GaussianAdapter": "gaussian_adapter", "GaussianAdapterCfg": "gaussian_adapter",
         "Gaussians": "gaussian_adapter", "DepthPredictorMonocular": "depth_head", "opacity_exponent": "depth_head",
         "Scene3DGS": "ply_import", "load_ply": "ply_import", "unpack_vertices": "ply_import",
         "pack_scene": "ply_export", "save_ply": "ply_export", "save_gaussians": "ply_export",
         "GaussianScene": "scene_model", "activate_scene": "scene_model",
         "photometric_loss": "losses", "ssim": "losses", "l1": "losses", "compute_ssim": "losses",
         "accumulate_density_stats": "density", "plan_densify": "density", "apply_densify": "density",
         "DensityControl": "density",
         "MCMCControl": "mcmc", "sample_by_weight": "mcmc", "relocation_values": "mcmc", "inject_noise": "mcmc",
         "compute_filter_3d": "filter3d", "activate_scene_filtered": "filter3d", "fused_parameters": "filter3d",
         "bilagrid_slice": "bilagrid", "bilagrid_tv": "bilagrid", "BilateralGrid": "bilagrid",
         "knn3": "knn", "mean_knn_dist2": "knn", "load_points_ply": "ply_import",
         "similarity_matrix": "transform", "invert_similarity": "transform", "transform_records": "transform",
         "transform_scene": "transform", "transform_cameras": "transform",
         "pose_matrices": "pose", "pose_scene": "pose", "PartPoses": "pose",
         "vq_assign": "vq", "vq_update": "vq", "kmeans": "vq", "quantize_scene": "vq", "QuantizedScene": "vq",
         "contribution_weights": "vq",
         "gaussian_normals": "normals", "normal_consistency_loss": "normals", "depth_to_normals": "normals",
         "flatten_loss": "normals",
         "TSDFVolume": "mesh", "save_mesh_ply": "mesh", "load_mesh_ply": "mesh",
         "mesh_components": "mesh", "clean_mesh": "mesh",
         "NearestIndex": "nn", "nearest": "nn",
         "cloud_metrics": "mesh_eval", "sample_mesh": "mesh_eval",
         "prepare_images": "images", "SourceCamera": "images",
         "inverse_depth_loss": "depth_sup", "sparse_inverse_depth": "depth_sup", "align_depth_prior": "depth_sup",
         "load_depth_prior": "depth_sup", "prepare_depth_priors": "depth_sup",
         "gaussian_depth_moments": "distortion", "distortion_loss": "distortion", "distortion_map": "distortion",
         "depth_pivot": "distortion",
         "Capture": "capture", "read_colmap_model": "capture", "ColmapModel": "capture",
         "adam_step": "optim", "SceneAdam": "optim", "expon_lr": "optim", "visible_from_radii": "optim"}


def __getattr__(name):     # torch is imported only when one of these is first used
    if name in _LAZY:
        from importlib import import_module
        return getattr(import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
