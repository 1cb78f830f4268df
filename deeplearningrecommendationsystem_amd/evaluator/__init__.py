from .evaluator import Evaluator
from .ranking import Ranking, RankingMetrics, itemid_matrix, ranking_metrics, ranking_partials, remove_itemid

__all__ = ["Evaluator", "Ranking", "RankingMetrics", "itemid_matrix", "ranking_metrics", "ranking_partials", "remove_itemid"]
