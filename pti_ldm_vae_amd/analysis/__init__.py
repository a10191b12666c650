"""Latent-space analysis of a trained VAE (reference ``src/pti_ldm_vae/analysis``): cached deterministic encodes, PCA /
t-SNE / UMAP projections and per-patient distance statistics between two image groups, with the distance, statistics
and Gram-matrix arithmetic on the device (``ops.latent_pairwise`` / ``ops.latent_group_stats``), a quality report of a
projection (``projection_quality``: trustworthiness, continuity, label separation) and its co-ranking curves and Shepard
figure (``coranking_curves``: Q_NX, B_NX, R_NX, LCMC for every neighbourhood size, stress), and permutation tests of whether
two groups of rows differ by more than chance (``two_sample_tests``: MMD^2, energy distance, neighbour share).  The reference's
image-comparison class (cv2, skimage, VGG) is not part of this package."""
from .coranking import coranking_curves
from .latent_cache import LatentCache
from .latent_distance import latent_distance, latent_distance_cross, latent_distance_from_indices
from .latent_space import (LatentSpaceAnalyzer, compute_distance_metrics, extract_patient_id_from_filename, load_image_paths)
from .projection_quality import projection_quality
from .two_sample import permutation_masks, two_sample_tests

__all__ = ["LatentCache", "LatentSpaceAnalyzer", "compute_distance_metrics", "coranking_curves",
           "extract_patient_id_from_filename", "latent_distance", "latent_distance_cross", "latent_distance_from_indices",
           "load_image_paths", "permutation_masks", "projection_quality", "two_sample_tests"]
