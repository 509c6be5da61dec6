from gen_adversarial_amd.experiments.alpha_learning.common_utils import (DEFENDERS, ROW_BUDGET, AlphaEvaluator,  # noqa: F401
                                                                          get_best_combination, get_cosine_alphas, get_linear_alphas,
                                                                          random_search)
