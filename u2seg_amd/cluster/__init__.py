from . import dino, kmeans, knn, select
from .dino import DinoViT, get_feats_list, load_dino_weights, vit_base, vit_small

__all__ = ["DinoViT", "dino", "get_feats_list", "kmeans", "knn", "load_dino_weights", "select", "vit_base", "vit_small"]
