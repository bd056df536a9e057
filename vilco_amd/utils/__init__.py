from .nms import batched_nms, nms_1d_cpu  # noqa: F401
from .train_utils import (fix_random_seed, make_optimizer, make_scheduler, save_checkpoint,  # noqa: F401
                          train_step)
from .metrics import ANETdetection  # noqa: F401
from .metrics_nlq import (NLQRecordStream, ReferringRecall, evaluate_nlq_performance,  # noqa: F401
                          make_nlq_evaluator)
from .ensemble_nlq import (NLQEnsembleStream, ensemble_predictions, ensemble_streams, nlq_ensemble_device,  # noqa: F401
                           temporal_nms, top1_generator)
from .postprocessing import (fuse_external_scores, load_results_from_json, load_results_from_pkl,  # noqa: F401
                             postprocess_results, results_to_array, results_to_dict)
