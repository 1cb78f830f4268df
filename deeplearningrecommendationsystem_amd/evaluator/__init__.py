from .evaluator import Evaluator
from .ranking import Ranking, RankingMetrics, itemid_matrix, ranking_metrics, ranking_partials, remove_itemid
from .sampled import GroupRankingMetrics, group_histogram, group_ranking_metrics, group_ranks
from .score import GaucResult, ScoreMetrics, UserGroups, gauc_from_counts, score_metrics, user_auc_counts

__all__ = ["Evaluator", "Ranking", "RankingMetrics", "itemid_matrix", "ranking_metrics", "ranking_partials", "remove_itemid",
           "GroupRankingMetrics", "group_histogram", "group_ranking_metrics", "group_ranks",
           "GaucResult", "ScoreMetrics", "UserGroups", "gauc_from_counts", "score_metrics", "user_auc_counts"]
