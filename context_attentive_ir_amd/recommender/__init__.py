"""Recommender models on the HIP path (mirror of /root/reference/neuroir/recommender): Seq2seq, HredQS, ACG."""
from .acg import ACG
from .hredqs import HredQS
from .seq2seq import Seq2seq

__all__ = ["Seq2seq", "HredQS", "ACG"]
