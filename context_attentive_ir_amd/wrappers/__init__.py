from .ranker import Ranker
from .multitask import Multitask
from .recommender import CopyRecommender, Recommender, SessionRecommender
from .common import GraphedUpdate

__all__ = ["Ranker", "Multitask", "Recommender", "SessionRecommender", "CopyRecommender", "GraphedUpdate"]
