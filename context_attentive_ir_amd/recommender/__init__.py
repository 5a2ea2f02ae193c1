"""Recommender models on the HIP path (mirror of /root/reference/neuroir/recommender): Seq2seq, HredQS, ACG, and the GRU-decoder forms of the
two attention recommenders."""
from .acg import ACG
from .hredqs import HredQS
from .seq2seq import Seq2seq
from .seq2seq_gru import ACGGRU, Seq2seqGRU

__all__ = ["Seq2seq", "HredQS", "ACG", "Seq2seqGRU", "ACGGRU"]
