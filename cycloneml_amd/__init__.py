"""cycloneml_amd -- MI355X (gfx950) backend for the MLlib linear-algebra hot
path of wmeddie/CycloneML: KMeans findClosest/cluster sums, the logistic
block aggregators, RowMatrix Gramian/covariance, and the treeAggregate merge
as an RCCL all-reduce.  Kernels live in libcyclone.so (csrc/, C ABI in
include/cyclone.h); these modules mirror the reference's Scala interfaces.
"""
__version__ = "0.1.0"

from . import _native  # noqa: F401  (loads nothing until first use)
from .bisecting_kmeans import (  # noqa: F401
    BisectingKMeans,
    BisectingKMeansModel,
    BKMPlan,
)
from .classification import (  # noqa: F401
    MultilayerPerceptronClassificationModel,
    MultilayerPerceptronClassifier,
    NaiveBayes,
    NaiveBayesModel,
)
from .feature import PCA, PCAModel  # noqa: F401
from .gmm import (  # noqa: F401
    GaussianMixture,
    GaussianMixtureModel,
    GMMPlan,
    MultivariateGaussian,
)
from .glm import (  # noqa: F401
    GeneralizedLinearRegression,
    GeneralizedLinearRegressionModel,
    IterativelyReweightedLeastSquares,
)
from .recommendation import ALS, ALSModel, ALSPlan  # noqa: F401
from .regression import (  # noqa: F401
    LinearRegression,
    LinearRegressionModel,
    SingularMatrixException,
    WeightedLeastSquares,
    WeightedLeastSquaresModel,
)
from .tree import (  # noqa: F401
    DecisionTreeClassificationModel,
    DecisionTreeClassifier,
    DecisionTreeRegressionModel,
    DecisionTreeRegressor,
    DTPlan,
)
from .forest import (  # noqa: F401
    RandomForestClassificationModel,
    RandomForestClassifier,
    RandomForestRegressionModel,
    RandomForestRegressor,
    RFPlan,
)
from .gbt import (  # noqa: F401
    GBTClassificationModel,
    GBTClassifier,
    GBTPlan,
    GBTRegressionModel,
    GBTRegressor,
)
from .regression_summary import (  # noqa: F401
    LinearRegressionSummary,
    LinearRegressionTrainingSummary,
)
