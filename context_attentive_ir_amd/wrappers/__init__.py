from .ranker import Ranker
from .multitask import Multitask
from .recommender import Recommender, SessionRecommender
from .common import GraphedUpdate

__all__ = ["Ranker", "Multitask", "Recommender", "SessionRecommender", "GraphedUpdate"]
