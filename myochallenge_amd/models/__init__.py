from .classifier import (DIMS_PER_OBS, N_OBS_PER_TRIAL, DataCollector, TaskClassifier, collect_data_for_classifier,  # noqa: F401
                         load_scaler, train_task_classifier)
